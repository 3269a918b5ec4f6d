// Uniform_Topology / Nonuniform_Topology for many problems in one GPU pass (desc_models_batch_*): the generator in front of the *_batch
// solvers of a Monte-Carlo study.  The definition of the draws -- keys, streams, which component is which matrix entry -- stands in
// include/desc_amd.h; tests/models_batch_oracle.py restates it in NumPy.
//
// The problems lie behind one another, as in cemp_batch.hip: global node g = node_off[b] + v, global edge edge_off[b] + e.
//
//   k_mb_rows<0> one wave per (problem, row i): lanes stride over j > i, evaluate the pair keys, ballot + popcount count the row's edges
//   k_mb_scan    one wave per problem: exclusive scan of the row counts -> row offsets, and the problem's edge count m_b
//                -- the host reads the B edge counts, the only sizes it needs, and allocates the edge arrays --
//   k_mb_rows<1> the rows again: the same keys, edge (i, j) written at edge_off + row offset + prefix popcount: sorted by (i, j) without
//                a sort, and no n x n array anywhere
//   k_mb_nodes   one thread per (problem, node): R_orig and R_corr / R_crpt
//   k_mb_mark    Nonuniform: one wave per node ranks the node's key among its problem's; the floor(n p_node_crpt) smallest are corrupted
//   k_mb_select  Nonuniform: one workgroup per corrupted node v ranks the keys of v's incident edges by counting; the incident edges
//                are found by binary search in the sorted rows (edge {x, v} lies in row min(x, v)); candidates are staged in LDS
//                MB_CHUNK at a time, a row longer than that is strided.  Writes sel_lo[e] / sel_hi[e]: edge e was selected by its first /
//                second node -- two arrays, so that the two endpoints' workgroups never write one byte
//   k_mb_edges   one thread per edge: Rij_orig = R_i R_j', the edge's decision (the winner of a doubly selected edge is the endpoint with
//                the larger node key), the normal block, the projection, ErrVec and the corrupted flag.  The 72-byte blocks are staged
//                in LDS and written by consecutive lanes to consecutive doubles: a wave's stores cover whole lines
//
// Composition independence.  Every key takes the problem's seed and an id counted inside the problem; a problem's ranks run over its own
// nodes and rows.  Which workgroup runs an item, and what else the batch holds, enters no result.
//
// Control flow.  No grid-wide barrier, no spinning on memory, no atomics.  Every loop is bounded by n, a row length or MB_CHUNK.  The
// workgroup barriers of k_mb_select, k_mb_nodes and k_mb_edges are reached by all 256 threads: their conditions are workgroup-uniform.
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "batch_device.h"
#include "cemp_math.h"
#include "problem_batch.h"
#include "so3_blocks.h"

namespace desc {
namespace {

constexpr int MB_MAX_N = 65536;                 // n (n - 1) / 2 < 2^31
constexpr int MB_CHUNK = 1024;                  // candidates k_mb_select stages in LDS at a time
constexpr double MB_TWO_PI = 6.283185307179586;

struct MbProb {
    int32_t kind, n, mode, ncrpt;               // ncrpt: floor(n * p_node_crpt)
    int32_t node_off, edge_off, m, pad;         // edge_off, m: filled in after the graph pass
    double p, q, p_edge, sig_a, sig_b;          // sig_a: sigma | sigma_in, sig_b: sigma_out
    uint64_t seed;
};

struct MbArgs {
    const MbProb* prob = nullptr;
    const int32_t* nprob = nullptr;             // N: the problem of a global node
    int32_t *rowcnt = nullptr, *rowoff = nullptr, *mcount = nullptr;      // N, N (local to the problem), B
    int32_t *ii = nullptr, *jj = nullptr, *eprob = nullptr;               // M each
    double *r_orig = nullptr, *r2 = nullptr;                              // N x 9
    uint8_t *crpt = nullptr, *sel_lo = nullptr, *sel_hi = nullptr;        // N, M, M (Nonuniform only)
    double *rij = nullptr, *rij_orig = nullptr, *err = nullptr;           // M x 9, M x 9, M
    uint8_t* corrupted = nullptr;                                         // M
    int32_t B = 0, N = 0, M = 0;
};

__device__ __forceinline__ double mb_uniform(uint64_t key) { return (double)(key >> 11) * 0x1p-53; }
// normal draw c of (stream key sk, id)
__device__ __forceinline__ double mb_normal(uint64_t sk, uint64_t id, uint64_t c) {
    const uint64_t k1 = d_sample_key(sk, id, 2 * c), k2 = d_sample_key(sk, id, 2 * c + 1);
    const double u1 = ((double)(k1 >> 12) + 0.5) * 0x1p-52, u2 = (double)(k2 >> 11) * 0x1p-53;
    return sqrt(-2.0 * log(u1)) * cos(MB_TWO_PI * u2);
}
__device__ __forceinline__ void mb_normal_block(uint64_t sk, uint64_t id, double* q) {
    for (int c = 0; c < 9; ++c) q[c] = mb_normal(sk, id, (uint64_t)c);
}

// A B' of two column-major blocks: out(r, c) = sum_k A(r, k) B(c, k)
__device__ __forceinline__ void mb_mul_abt(const double* A, const double* Bm, double* out) {
    for (int c = 0; c < 3; ++c)
        for (int r = 0; r < 3; ++r) {
            double acc = 0.0;
            for (int k = 0; k < 3; ++k) acc += A[r + 3 * k] * Bm[c + 3 * k];
            out[r + 3 * c] = acc;
        }
}

// pass 1 (FILL = false) and pass 2 (FILL = true) over the rows of the upper triangle
template <bool FILL>
__global__ __launch_bounds__(256) void k_mb_rows(MbArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t g64 = wid; g64 < a.N; g64 += nw) {
        const int g = __builtin_amdgcn_readfirstlane((int)g64);
        const int b = uniform_load(a.nprob, g);
        const MbProb pd = a.prob[b];
        const int i = g - pd.node_off, n = pd.n;
        const uint64_t sk = d_sample_key(pd.seed, DESC_MODELS_STREAM_EDGE, 0);
        const uint64_t base = (uint64_t)i * (uint64_t)n - (uint64_t)i * (uint64_t)(i + 1) / 2;       // t of the pair (i, i + 1)
        const int64_t out0 = FILL ? (int64_t)pd.edge_off + a.rowoff[g] : 0;
        int cnt = 0;
        for (int j0 = i + 1; j0 < n; j0 += 64) {
            const int j = j0 + lane;
            const bool edge = j < n && mb_uniform(d_sample_key(sk, base + (uint64_t)(j - i - 1), 0)) < pd.p;
            const unsigned long long mk = __ballot(edge);
            if (FILL && edge) {
                const int64_t pos = out0 + cnt + __popcll(mk & ((1ull << lane) - 1ull));
                a.ii[pos] = i; a.jj[pos] = j; a.eprob[pos] = b;
            }
            cnt += __popcll(mk);
        }
        if (!FILL && lane == 0) a.rowcnt[g] = cnt;
    }
}

__global__ __launch_bounds__(64) void k_mb_scan(MbArgs a) {
    const int lane = threadIdx.x;
    for (int b = blockIdx.x; b < a.B; b += gridDim.x) {
        const MbProb pd = a.prob[b];
        int carry = 0;
        for (int v0 = 0; v0 < pd.n; v0 += 64) {
            const int v = v0 + lane;
            const int c = v < pd.n ? a.rowcnt[pd.node_off + v] : 0;
            int incl = c;
            for (int d = 1; d < 64; d <<= 1) { const int t = __shfl_up(incl, d); if (lane >= d) incl += t; }
            if (v < pd.n) a.rowoff[pd.node_off + v] = carry + incl - c;
            carry += __shfl(incl, 63);
        }
        if (lane == 0) a.mcount[b] = carry;
    }
}

__global__ __launch_bounds__(256) void k_mb_nodes(MbArgs a) {
    __shared__ double stage[256 * 9];
    const int first = (int)blockIdx.x * 256, g = first + (int)threadIdx.x;
    const int nvalid = min(256, a.N - first);
    double q[9], R[9], R2[9];
    for (int k = 0; k < 9; ++k) { R[k] = 0.0; R2[k] = 0.0; }
    if (g < a.N) {
        const MbProb pd = a.prob[a.nprob[g]];
        const uint64_t v = (uint64_t)(g - pd.node_off);
        mb_normal_block(d_sample_key(pd.seed, DESC_MODELS_STREAM_RORIG, 0), v, q);
        mb_project(q, R);
        mb_normal_block(d_sample_key(pd.seed, DESC_MODELS_STREAM_RCORR, 0), v, q);
        mb_project(q, R2);
    }
    mb_store_blocks(stage, a.r_orig + 9 * (int64_t)first, R, nvalid);
    mb_store_blocks(stage, a.r2 + 9 * (int64_t)first, R2, nvalid);
}

__global__ __launch_bounds__(256) void k_mb_mark(MbArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6, nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t g64 = wid; g64 < a.N; g64 += nw) {
        const int g = __builtin_amdgcn_readfirstlane((int)g64);
        const MbProb pd = a.prob[uniform_load(a.nprob, g)];
        int rank = 0;
        const bool take = pd.kind == DESC_MODELS_KIND_NONUNIFORM && pd.ncrpt > 0;
        if (take) {
            const int v = g - pd.node_off;
            const uint64_t sk = d_sample_key(pd.seed, DESC_MODELS_STREAM_NODE, 0);
            const uint64_t kv = d_sample_key(sk, (uint64_t)v, 0);
            for (int u0 = 0; u0 < pd.n; u0 += 64) {
                const int u = u0 + lane;
                bool before = false;
                if (u < pd.n) { const uint64_t ku = d_sample_key(sk, (uint64_t)u, 0); before = ku < kv || (ku == kv && u < v); }
                rank += __popcll(__ballot(before));
            }
        }
        if (lane == 0) a.crpt[g] = (take && rank < pd.ncrpt) ? 1 : 0;
    }
}

// local id of the edge {x, v} of problem pd (x != v), -1 if the pair is no edge: binary search for max(x, v) in row min(x, v)
__device__ __forceinline__ int mb_find_edge(const MbArgs& a, const MbProb& pd, int x, int v) {
    const int lo_node = x < v ? x : v, hi_node = x < v ? v : x;
    int lo = a.rowoff[pd.node_off + lo_node], hi = lo + a.rowcnt[pd.node_off + lo_node];
    const int32_t* jj = a.jj + pd.edge_off;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        const int j = jj[mid];
        if (j == hi_node) return mid;
        if (j < hi_node) lo = mid + 1; else hi = mid;
    }
    return -1;
}

__global__ __launch_bounds__(256) void k_mb_select(MbArgs a) {
    __shared__ uint64_t ckey[MB_CHUNK];
    __shared__ int32_t cid[MB_CHUNK];
    const int tid = threadIdx.x;
    for (int g = blockIdx.x; g < a.N; g += gridDim.x) {                  // every condition below is the same in all 256 threads
        if (!a.crpt[g]) continue;
        const MbProb pd = a.prob[a.nprob[g]];
        const int v = g - pd.node_off, n = pd.n;
        const uint64_t sk = d_sample_key(pd.seed, DESC_MODELS_STREAM_SELECT, (uint64_t)v);
        // candidates c0 .. c0 + MB_CHUNK - 1 (the other endpoint x) into LDS; returns how many of them are edges
        auto fill = [&](int c0) -> int {
            int cnt = 0;
            __syncthreads();                                             // the chunk's last readers are done
            for (int t = tid; t < MB_CHUNK; t += 256) {
                const int x = c0 + t;
                const int e = (x < n && x != v) ? mb_find_edge(a, pd, x, v) : -1;
                cid[t] = e;
                ckey[t] = e >= 0 ? d_sample_key(sk, (uint64_t)e, 0) : 0;
                cnt += __syncthreads_count(e >= 0);
            }
            return cnt;
        };
        int deg = 0;
        for (int c0 = 0; c0 < n; c0 += MB_CHUNK) deg += fill(c0);
        const int nsel = (int)floor(pd.p_edge * (double)deg);            // :80
        const bool resident = n <= MB_CHUNK;                             // the one chunk is still in LDS
        if (nsel > 0)
            for (int x0 = 0; x0 < n; x0 += 256) {
                const int x = x0 + tid;
                const int e = (x < n && x != v) ? mb_find_edge(a, pd, x, v) : -1;
                const uint64_t k = e >= 0 ? d_sample_key(sk, (uint64_t)e, 0) : 0;
                int rank = 0;
                for (int c0 = 0; c0 < n; c0 += MB_CHUNK) {
                    if (!resident) fill(c0);
                    const int len = min(MB_CHUNK, n - c0);
                    if (e >= 0)
                        for (int t = 0; t < len; ++t) {
                            const int e2 = cid[t];
                            const uint64_t k2 = ckey[t];
                            rank += (e2 >= 0 && (k2 < k || (k2 == k && e2 < e))) ? 1 : 0;
                        }
                }
                if (e >= 0 && rank < nsel) {
                    if (v < x) a.sel_lo[(int64_t)pd.edge_off + e] = 1; else a.sel_hi[(int64_t)pd.edge_off + e] = 1;
                }
            }
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void k_mb_edges(MbArgs a) {
    __shared__ double stage[256 * 9];
    const int64_t first = (int64_t)blockIdx.x * 256, g = first + threadIdx.x;
    const int nvalid = (int)min((int64_t)256, (int64_t)a.M - first);
    double Ro[9], R[9];
    for (int k = 0; k < 9; ++k) { Ro[k] = 0.0; R[k] = 0.0; }
    if (g < a.M) {
        const MbProb pd = a.prob[a.eprob[g]];
        const uint64_t e = (uint64_t)(g - pd.edge_off);
        const int i = a.ii[g], j = a.jj[g];
        const double* rn = a.r_orig + 9 * (int64_t)pd.node_off;
        const double* r2 = a.r2 + 9 * (int64_t)pd.node_off;
        double Ri[9], Rj[9], Q[9], N[9];
        load_block9(rn + 9 * i, Ri);
        load_block9(rn + 9 * j, Rj);
        mb_mul_abt(Ri, Rj, Ro);                                                          // :48-51
        bool bad;
        double sig;
        const uint64_t sk_noise = d_sample_key(pd.seed, DESC_MODELS_STREAM_NOISE, 0);
        if (pd.kind == DESC_MODELS_KIND_UNIFORM) {
            bad = !(mb_uniform(d_sample_key(d_sample_key(pd.seed, DESC_MODELS_STREAM_CORRUPT, 0), e, 0)) >= pd.q);      // :53
            sig = pd.sig_a;
            if (!bad) {
                for (int k = 0; k < 9; ++k) Q[k] = Ro[k];                                // :58-59
            } else if (pd.mode == DESC_MODELS_UNIFORM) {                                 // :76-82
                mb_normal_block(d_sample_key(pd.seed, DESC_MODELS_STREAM_HAAR, 0), e, Q);      // no noise on top: the block is projected as it is
            } else {                                                                     // :84-90
                double Ci[9], Cj[9];
                load_block9(r2 + 9 * i, Ci);
                load_block9(r2 + 9 * j, Cj);
                mb_mul_abt(Ci, Cj, Q);
            }
            if (!(bad && pd.mode == DESC_MODELS_UNIFORM)) {
                mb_normal_block(sk_noise, e, N);
                for (int k = 0; k < 9; ++k) Q[k] = Q[k] + sig * N[k];
            }
        } else {
            const bool by_i = a.sel_lo[g] != 0, by_j = a.sel_hi[g] != 0;
            bad = by_i || by_j;
            for (int k = 0; k < 9; ++k) Q[k] = Ro[k];
            if (bad) {
                bool w_is_i = by_i;
                if (by_i && by_j) {                                                      // the later node of the order overwrites (:76)
                    const uint64_t skn = d_sample_key(pd.seed, DESC_MODELS_STREAM_NODE, 0);
                    w_is_i = d_sample_key(skn, (uint64_t)i, 0) > d_sample_key(skn, (uint64_t)j, 0);        // equal keys: j > i is later
                }
                const int w = w_is_i ? i : j, x = w_is_i ? j : i;
                double Mw[9];
                if (pd.mode == DESC_MODELS_UNIFORM) {                                    // :88-99
                    double Z[9];
                    mb_normal_block(d_sample_key(pd.seed, DESC_MODELS_STREAM_R0, (uint64_t)w), e, Z);
                    mb_project(Z, Mw);
                } else {                                                                 // :101-115
                    double Cw[9], Xx[9];
                    load_block9(r2 + 9 * w, Cw);
                    load_block9((pd.mode == DESC_MODELS_SELF_CONSISTENT ? r2 : rn) + 9 * x, Xx);
                    mb_mul_abt(Cw, Xx, Mw);
                }
                for (int c = 0; c < 3; ++c)
                    for (int r = 0; r < 3; ++r) Q[r + 3 * c] = w_is_i ? Mw[r + 3 * c] : Mw[c + 3 * r];     // IndMat < 0: the transpose
            }
            sig = bad ? pd.sig_b : pd.sig_a;                                             // :121-127
            mb_normal_block(sk_noise, e, N);
            for (int k = 0; k < 9; ++k) Q[k] = Q[k] + sig * N[k];
        }
        mb_project(Q, R);
        double tr = 0.0;
        for (int k = 0; k < 9; ++k) tr += Ro[k] * R[k];
        a.err[g] = abs_acos_ext_c((tr - 1.0) / 2.0) / M_PI;
        a.corrupted[g] = bad ? 1 : 0;
    }
    mb_store_blocks(stage, a.rij_orig + 9 * first, Ro, nvalid);
    mb_store_blocks(stage, a.rij + 9 * first, R, nvalid);
}

__global__ void k_mb_test_draws(uint64_t seed, uint64_t stream, uint64_t sub, uint64_t id0, int64_t count, uint64_t c, int normal, double* out) {
    const uint64_t sk = d_sample_key(seed, stream, sub);
    for (int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; t < count; t += (int64_t)gridDim.x * blockDim.x)
        out[t] = normal ? mb_normal(sk, id0 + (uint64_t)t, c) : mb_uniform(d_sample_key(sk, id0 + (uint64_t)t, c));
}

}  // namespace
}  // namespace desc

using namespace desc;

struct desc_models_batch : BatchDevice {
    int32_t count = 0;
    bool any_nonuniform = false, generated = false;
    hvec<MbProb> pr;
    hvec<int64_t> m_per;
    MbArgs a;
    double ms_graph = 0;
};

namespace {

bool mb_prob_ok(double x) { return std::isfinite(x) && x >= 0.0 && x <= 1.0; }
bool mb_sigma_ok(double x) { return std::isfinite(x) && x >= 0.0; }

int mb_validate(const desc_model_spec* specs, int32_t count, hvec<MbProb>& pr, bool* any_nonuniform) {
    int64_t N = 0;
    double expected = 0.0;
    pr.resize((size_t)count);
    for (int32_t b = 0; b < count; ++b) {
        const desc_model_spec& s = specs[b];
        if (s.kind != DESC_MODELS_KIND_UNIFORM && s.kind != DESC_MODELS_KIND_NONUNIFORM)
            return fail(DESC_ERR_INVALID, "problem %d: unknown kind %d", b, (int)s.kind);
        const bool nu = s.kind == DESC_MODELS_KIND_NONUNIFORM;
        if (s.n < 2) return fail(DESC_ERR_INVALID, "problem %d: n = %d, need n >= 2", b, (int)s.n);
        if (s.n > MB_MAX_N) return fail(DESC_ERR_INVALID, "problem %d: n = %d exceeds %d", b, (int)s.n, MB_MAX_N);
        if (!mb_prob_ok(s.p)) return fail(DESC_ERR_INVALID, "problem %d: p must be a probability in [0, 1]", b);
        if (!nu && !mb_prob_ok(s.q)) return fail(DESC_ERR_INVALID, "problem %d: q must be a probability in [0, 1]", b);
        if (nu && !mb_prob_ok(s.p_node_crpt)) return fail(DESC_ERR_INVALID, "problem %d: p_node_crpt must be a probability in [0, 1]", b);
        if (nu && !mb_prob_ok(s.p_edge_crpt)) return fail(DESC_ERR_INVALID, "problem %d: p_edge_crpt must be a probability in [0, 1]", b);
        if (!nu && !mb_sigma_ok(s.sigma)) return fail(DESC_ERR_INVALID, "problem %d: sigma must be finite and >= 0", b);
        if (nu && !mb_sigma_ok(s.sigma_in)) return fail(DESC_ERR_INVALID, "problem %d: sigma_in must be finite and >= 0", b);
        if (nu && !mb_sigma_ok(s.sigma_out)) return fail(DESC_ERR_INVALID, "problem %d: sigma_out must be finite and >= 0", b);
        if (nu && s.mode != DESC_MODELS_UNIFORM && s.mode != DESC_MODELS_SELF_CONSISTENT && s.mode != DESC_MODELS_ADV)
            return fail(DESC_ERR_INVALID, "problem %d: unknown mode %d", b, (int)s.mode);
        MbProb& q = pr[(size_t)b];
        std::memset(&q, 0, sizeof(q));
        q.kind = s.kind; q.n = s.n; q.node_off = (int32_t)N; q.p = s.p; q.seed = s.seed;
        if (nu) {
            q.mode = s.mode; q.ncrpt = (int32_t)std::floor((double)s.n * s.p_node_crpt);
            q.p_edge = s.p_edge_crpt; q.sig_a = s.sigma_in; q.sig_b = s.sigma_out;
            *any_nonuniform = true;
        } else {
            q.mode = s.mode == DESC_MODELS_UNIFORM ? DESC_MODELS_UNIFORM : DESC_MODELS_SELF_CONSISTENT;
            q.q = s.q; q.sig_a = s.sigma;
        }
        N += s.n;
        expected += s.p * (0.5 * (double)s.n * (double)(s.n - 1));
        if (N >= (1ll << 31)) return fail(DESC_ERR_TOO_LARGE, "the batch holds 2^31 nodes or more at problem %d: split the batch", b);
        if (expected >= (double)(1ll << 30))
            return fail(DESC_ERR_TOO_LARGE, "the batch is expected to draw 2^30 edges or more at problem %d (152 bytes each): split the batch", b);
    }
    return DESC_OK;
}

int mb_create(const desc_model_spec* specs, int32_t count, int32_t device, desc_models_batch* h) {
    auto t0 = std::chrono::steady_clock::now();
    h->count = count;
    int rc = mb_validate(specs, count, h->pr, &h->any_nonuniform);
    if (rc) return rc;
    h->m_per.assign((size_t)count, 0);
    if (count == 0) return DESC_OK;

    if ((rc = h->open(device, "the batched model generator"))) return rc;              // nothing above touched the device
    MbArgs& a = h->a;
    const size_t B = (size_t)count, N = (size_t)h->pr.back().node_off + (size_t)h->pr.back().n;
    hvec<int32_t> nprob(N);
    for (size_t b = 0; b < B; ++b) std::fill(nprob.begin() + h->pr[b].node_off, nprob.begin() + h->pr[b].node_off + h->pr[b].n, (int32_t)b);
    MbProb* d_prob = nullptr;
    if ((rc = h->upload(&d_prob, h->pr.data(), B)) || (rc = h->upload(&a.nprob, nprob.data(), N)) ||
        (rc = h->mem.alloc(&a.rowcnt, N)) || (rc = h->mem.alloc(&a.rowoff, N)) || (rc = h->mem.alloc(&a.mcount, B))) return rc;
    a.prob = d_prob; a.B = count; a.N = (int32_t)N;
    // ---- pass 1: row counts, row offsets, the problems' edge counts
    hipLaunchKernelGGL(k_mb_rows<false>, dim3((unsigned)grid_for((int64_t)N, 16384, 4)), dim3(256), 0, h->stream, a);
    hipLaunchKernelGGL(k_mb_scan, dim3((unsigned)grid_for((int64_t)B, 4096, 1)), dim3(64), 0, h->stream, a);
    DESC_HIP(hipGetLastError());
    hvec<int32_t> mcount(B);
    DESC_HIP(hipMemcpyAsync(mcount.data(), a.mcount, sizeof(int32_t) * B, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipStreamSynchronize(h->stream));                                          // nprob goes out of scope below; the B sizes
    int64_t M = 0;
    for (size_t b = 0; b < B; ++b) {
        if (mcount[b] < 0 || (int64_t)mcount[b] > (int64_t)h->pr[b].n * (h->pr[b].n - 1) / 2)
            return fail(DESC_ERR_STATE, "problem %d: the graph pass counted %d edges", (int)b, (int)mcount[b]);
        h->pr[b].edge_off = (int32_t)M; h->pr[b].m = mcount[b]; h->m_per[b] = mcount[b];
        M += mcount[b];
        if (M >= (1ll << 31) - 256) return fail(DESC_ERR_TOO_LARGE, "the batch drew 2^31 edges or more at problem %d: split the batch", (int)b);
    }
    a.M = (int32_t)M;
    DESC_HIP(hipMemcpyAsync(d_prob, h->pr.data(), sizeof(MbProb) * B, hipMemcpyHostToDevice, h->stream));      // h->pr lives with the handle
    const size_t Ms = (size_t)M;
    if ((rc = h->mem.alloc(&a.ii, Ms)) || (rc = h->mem.alloc(&a.jj, Ms)) || (rc = h->mem.alloc(&a.eprob, Ms))) return rc;
    // ---- pass 2: the sorted edge list
    if (M > 0) hipLaunchKernelGGL(k_mb_rows<true>, dim3((unsigned)grid_for((int64_t)N, 16384, 4)), dim3(256), 0, h->stream, a);
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipStreamSynchronize(h->stream));
    h->ms_graph = ms_since(t0);
    return DESC_OK;
}

int mb_generate(desc_models_batch* h, double* ms_nodes, double* ms_edges) {
    MbArgs& a = h->a;
    const size_t N = (size_t)a.N, M = (size_t)a.M;
    int rc;
    auto t0 = std::chrono::steady_clock::now();
    if (!a.r_orig) {
        if ((rc = h->mem.alloc(&a.r_orig, 9 * N)) || (rc = h->mem.alloc(&a.r2, 9 * N)) || (rc = h->mem.alloc(&a.rij, 9 * M)) ||
            (rc = h->mem.alloc(&a.rij_orig, 9 * M)) || (rc = h->mem.alloc(&a.err, M)) || (rc = h->mem.alloc(&a.corrupted, M))) return rc;
        if (h->any_nonuniform && ((rc = h->mem.alloc(&a.crpt, N)) || (rc = h->mem.alloc(&a.sel_lo, M)) || (rc = h->mem.alloc(&a.sel_hi, M)))) return rc;
    }
    hipLaunchKernelGGL(k_mb_nodes, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, h->stream, a);
    if (h->any_nonuniform && M > 0) {
        DESC_HIP(hipMemsetAsync(a.sel_lo, 0, M, h->stream));
        DESC_HIP(hipMemsetAsync(a.sel_hi, 0, M, h->stream));
        hipLaunchKernelGGL(k_mb_mark, dim3((unsigned)grid_for((int64_t)N, 16384, 4)), dim3(256), 0, h->stream, a);
        hipLaunchKernelGGL(k_mb_select, dim3((unsigned)grid_for((int64_t)N, 65536, 1)), dim3(256), 0, h->stream, a);
    }
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipStreamSynchronize(h->stream));
    *ms_nodes = ms_since(t0);
    auto t1 = std::chrono::steady_clock::now();
    if (M > 0) hipLaunchKernelGGL(k_mb_edges, dim3((unsigned)((M + 255) / 256)), dim3(256), 0, h->stream, a);
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipStreamSynchronize(h->stream));
    *ms_edges = ms_since(t1);
    h->generated = true;
    return DESC_OK;
}

int mb_test_draws(const char* name, uint64_t seed, uint64_t stream, uint64_t sub, uint64_t id0, int64_t count, uint64_t c, int normal, int32_t device,
                  double* out) {
    return no_throw(name, [&]() -> int {
        if (!out || count < 0) return fail(DESC_ERR_INVALID, "NULL out or negative count");
        if (count == 0) return DESC_OK;
        BatchDevice dev;
        int rc = dev.open(device, "the model generator's draw hook");
        if (rc) return rc;
        double* d = nullptr;
        if ((rc = dev.mem.alloc(&d, (size_t)count))) return rc;
        hipLaunchKernelGGL(k_mb_test_draws, dim3((unsigned)grid_for(count, 4096)), dim3(256), 0, dev.stream, seed, stream, sub, id0, count, c, normal, d);
        DESC_HIP(hipGetLastError());
        DESC_HIP(hipMemcpyAsync(out, d, sizeof(double) * (size_t)count, hipMemcpyDeviceToHost, dev.stream));
        DESC_HIP(hipStreamSynchronize(dev.stream));
        return DESC_OK;
    });
}

}  // namespace

// For desc_problem_batch_from_models (problem_batch.hip): the node and edge passes run here if no fetch has run them yet; nothing is
// copied to the host.
int desc::models_batch_view(desc_models_batch* h, ModelsView* out) {
    out->count = h->count; out->device = h->device; out->m_per = h->m_per.data();
    if (h->count == 0) return DESC_OK;
    DESC_HIP(hipSetDevice(h->device));
    if (!h->generated) {
        double ms_nodes = 0, ms_edges = 0;
        const int rc = mb_generate(h, &ms_nodes, &ms_edges);
        if (rc) return rc;
    }
    DESC_HIP(hipStreamSynchronize(h->stream));
    out->d_ii = h->a.ii; out->d_jj = h->a.jj; out->d_rij = h->a.rij; out->M = h->a.M;
    return DESC_OK;
}

extern "C" {

uint64_t desc_models_key(uint64_t seed, uint64_t stream, uint64_t sub, uint64_t id, uint64_t c) {
    return sample_key(sample_key(seed, stream, sub), id, c);
}

int32_t desc_models_batch_max_n(void) { return MB_MAX_N; }

int desc_models_batch_create(const desc_model_spec* specs, int32_t count, int32_t device, desc_models_batch** out) {
    return batch_create_guarded("desc_models_batch_create", out, specs, count, [&](desc_models_batch* h) { return mb_create(specs, count, device, h); });
}

int desc_models_batch_sizes(const desc_models_batch* h, int64_t* m_per_problem) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    if (m_per_problem) for (int32_t b = 0; b < h->count; ++b) m_per_problem[b] = h->m_per[(size_t)b];
    return DESC_OK;
}

int desc_models_batch_fetch(desc_models_batch* h, int32_t* ind_i, int32_t* ind_j, double* rij, double* rij_orig, double* r_orig, double* err_vec,
                            uint8_t* corrupted, desc_models_batch_timings* tm) {
    return no_throw("desc_models_batch_fetch", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        auto t0 = std::chrono::steady_clock::now();
        if (tm) { tm->ms_graph = h->ms_graph; tm->ms_nodes = 0; tm->ms_edges = 0; tm->ms_copy = 0; tm->ms_total = h->ms_graph; }
        if (h->count == 0) return DESC_OK;
        DESC_HIP(hipSetDevice(h->device));
        double ms_nodes = 0, ms_edges = 0;
        int rc = mb_generate(h, &ms_nodes, &ms_edges);
        if (rc) return rc;
        auto t1 = std::chrono::steady_clock::now();
        const MbArgs& a = h->a;
        const size_t N = (size_t)a.N, M = (size_t)a.M;
        if (r_orig) DESC_HIP(hipMemcpyAsync(r_orig, a.r_orig, sizeof(double) * 9 * N, hipMemcpyDeviceToHost, h->stream));
        if (M > 0) {
            if (ind_i) DESC_HIP(hipMemcpyAsync(ind_i, a.ii, sizeof(int32_t) * M, hipMemcpyDeviceToHost, h->stream));
            if (ind_j) DESC_HIP(hipMemcpyAsync(ind_j, a.jj, sizeof(int32_t) * M, hipMemcpyDeviceToHost, h->stream));
            if (rij) DESC_HIP(hipMemcpyAsync(rij, a.rij, sizeof(double) * 9 * M, hipMemcpyDeviceToHost, h->stream));
            if (rij_orig) DESC_HIP(hipMemcpyAsync(rij_orig, a.rij_orig, sizeof(double) * 9 * M, hipMemcpyDeviceToHost, h->stream));
            if (err_vec) DESC_HIP(hipMemcpyAsync(err_vec, a.err, sizeof(double) * M, hipMemcpyDeviceToHost, h->stream));
            if (corrupted) DESC_HIP(hipMemcpyAsync(corrupted, a.corrupted, M, hipMemcpyDeviceToHost, h->stream));
        }
        DESC_HIP(hipStreamSynchronize(h->stream));
        if (tm) { tm->ms_nodes = ms_nodes; tm->ms_edges = ms_edges; tm->ms_copy = ms_since(t1); tm->ms_total = h->ms_graph + ms_since(t0); }
        return DESC_OK;
    });
}

void desc_models_batch_destroy(desc_models_batch* h) { delete h; }

int desc_test_models_uniform(uint64_t seed, uint64_t stream, uint64_t sub, uint64_t id0, int64_t count, uint64_t c, int32_t device, double* out) {
    return mb_test_draws("desc_test_models_uniform", seed, stream, sub, id0, count, c, 0, device, out);
}
int desc_test_models_normal(uint64_t seed, uint64_t stream, uint64_t sub, uint64_t id0, int64_t count, uint64_t c, int32_t device, double* out) {
    return mb_test_draws("desc_test_models_normal", seed, stream, sub, id0, count, c, 1, device, out);
}

}  // extern "C"

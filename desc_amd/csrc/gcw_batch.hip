// Spectral / GCW for many small problems in one GPU pass (desc_gcw_batch_*): the rotation step behind desc_pgd_batch_*.
//
// spectral.hip solves one problem per call with a host-driven loop: per outer step a Gram download, a 6x6 Jacobi on the host, a residual
// download and a coefficient upload -- a latency chain of a few milliseconds for a 100-node graph, whatever the card could do meanwhile.
// Here ONE launch solves all B problems: one workgroup of 256 threads per problem runs the whole Chebyshev-filtered subspace iteration of
// spectral_impl for its problem, from the start block to the Ritz vectors, without a host round trip.
//
// On-chip state.  The four 3n x 6 blocks (basis X, Y = A X, the two Chebyshev iterates) live in LDS, 576 n bytes, with 3.5 KiB of small
// matrices behind them (Grams, Ritz rotation, Cholesky coefficients, wave partials).  The LDS of a launch is sized from the largest
// problem of the batch; a problem addresses it with its own n, so nothing it computes depends on that size.  The cap GCW_BATCH_MAX_N is
// the largest n that fits the 160 KiB a workgroup may declare.
//
// Operator.  Each problem has its own CSR (local ids), the resident problem set's (problem_batch.h) the handle is created on.  The workgroup forms the weights 1/(S^1.5 + 1e-8),
// the weighted degrees, D^-1/2 and the 2m blocks w dinv_v dinv_u R (k_assemble_blocks of spectral.hip) once into global memory, 72
// contiguous bytes per slot, and reads them in every product.  The product gives thread (v, c) the three entries of node row v in column
// c: it walks the row's slots in CSR order with plain f64 FMAs -- no partial sums to combine, so the order of additions is the CSR's.
//
// Reductions.  Grams and residuals: thread t adds rows t, t + 256, ..., the 64 lanes of a wave are combined by the fixed butterfly
// (group_sum<64>), the waves 0..3 in order.  The 6x6 Jacobi and the Cholesky coefficients (small_dense.h, the text spectral.hip runs on
// the host) are computed by thread 0 between two barriers.
//
// Control flow.  Every thread evaluates the scheme's scalars (lo / cut / degree, the stop test) from the same LDS values with the same
// instructions, so all branches are uniform; the integers that steer loops and barriers go through readfirstlane.  Every loop is
// bounded by max_iters and the Chebyshev degree (<= 16); there is no grid-wide barrier, no spinning on memory and no communication
// between workgroups.  A problem that does not converge reports converged = 0.
//
// Composition independence.  Problem b's workgroup reads b's arrays and writes b's ranges; thread roles, loop bounds and summation
// orders are functions of b's n and CSR alone.  The tail (back-scaling by D^-1/2, unit columns, det sign, per-node projection onto
// SO(3)) runs per problem on host threads with the arithmetic of spectral.hip's tail (small_dense.h).
//
// Streamed blocks (k_gcw_batch<true>, opt-in: desc_gcw_batch_create_where).  Only the source block of a product is ever gathered from
// (x at adj[t]); y and z are touched at the thread's own elements, and Grams, combinations and residuals are straight row sweeps.  The
// streamed kernel therefore keeps the four blocks in a per-problem global workspace (72 n doubles at 72 node_off[b], L2-resident at these
// sizes) and LDS holds ONE staging block of 18 n doubles: a product first copies its source block there, takes a barrier, and gathers
// from LDS as before.  Operations, orders and reductions are those of the LDS kernel -- the same text on other pointers -- so a problem
// gets the same bits from either kernel, up to GCW_BATCH_STREAMED_MAX_N nodes.  A launch may cover a subset of the batch (GbArgs::list):
// with DESC_GCW_EIG_AUTO the problems that fit go to the LDS kernel and the others to the streamed one, two launches on one stream.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "batch_csr.h"
#include "batch_device.h"
#include "problem_batch.h"
#include "laa_wg.h"
#include "small_dense.h"

namespace desc {
namespace {

constexpr int BW = 6;                                   // block width of the subspace iteration (3 wanted + 3 guard vectors)
constexpr int GB_SCRATCH = 448;                         // doubles of small matrices behind the four blocks (see the offsets in the kernel)
constexpr int GB_LDS_BYTES = 160 * 1024;                // what one workgroup may declare on gfx950
constexpr int GCW_BATCH_MAX_N = (GB_LDS_BYTES / 8 - GB_SCRATCH) / (4 * 3 * BW);     // 278
static_assert(GCW_BATCH_MAX_N >= 200, "the Monte-Carlo sizes of the README must fit");
static_assert((4 * 3 * BW * GCW_BATCH_MAX_N + GB_SCRATCH) * 8 <= GB_LDS_BYTES, "LDS budget");

constexpr int GCW_BATCH_STREAMED_MAX_N = (GB_LDS_BYTES / 8 - GB_SCRATCH) / (3 * BW);      // 1112: one staging block in LDS
static_assert((3 * BW * GCW_BATCH_STREAMED_MAX_N + GB_SCRATCH) * 8 <= GB_LDS_BYTES, "LDS budget");
static_assert(GCW_BATCH_STREAMED_MAX_N >= REFINE_BATCH_MAX_N, "the streamed eigen-solve must start every problem the refinement takes");

inline size_t gb_lds_bytes(int n) { return sizeof(double) * ((size_t)4 * 3 * BW * (size_t)n + GB_SCRATCH); }

inline size_t gb_streamed_lds_bytes(int n) { return sizeof(double) * ((size_t)3 * BW * (size_t)n + GB_SCRATCH); }

struct GbInfo { int32_t iters, products, converged, status; double residual, eig[3]; };       // status: 1 degenerate start basis, 2 breakdown

struct GbArgs {
    const PbProb* prob;
    const int32_t* rowptr;      // problem b's n_b + 1 row starts at node_off[b] + b, counted inside the problem
    const int32_t* adj;         // 2 m_b local neighbour ids at 2 edge_off[b]
    const int32_t* adj_eid;     // 2 m_b local edge ids
    const double* rij;          // 9 m_b at 9 edge_off[b]
    const double* s_vec;        // GCW mode: S_vec of the whole batch, else NULL
    const double* wts_in;       // host weights of the whole batch, else NULL (both NULL: unit weights)
    double* w;                  // GCW mode: the weights formed here
    double* dinv;               // n_b at node_off[b]
    double* blocks;             // 18 m_b at 18 edge_off[b]: slot t of the problem at 9 t
    double* V;                  // 9 n_b at 9 node_off[b]: the three Ritz vectors, (3n x 3) row-major
    GbInfo* info;
    double* work;               // streamed kernel: X, Y, P, Q of problem b, 18 n_b doubles each, at 72 node_off[b]; else NULL
    const int32_t* list;        // the problems of this launch, one per workgroup; NULL: blockIdx.x is the problem
    double tol;
    int32_t normalize, max_iters;
};

// y[v] = alpha * sum_t blocks[t] * x[adj[t]] + s1 * x[v] + s2 * z[v]; x, y, z: (3n x BW) row-major in LDS, x != y (z may alias y: a
// thread reads exactly the elements it writes).  Thread (v, c) owns column c of node row v.  Ends with a barrier.
// STREAM: x, y, z are in global memory; x is first copied into the staging block `stage` (LDS, 18 n doubles; consecutive lanes take
// consecutive 16-byte pairs, every range being 16-byte aligned) and read from there.  The closing barrier also keeps the next product's
// copy off a staging block that is still being gathered from.
template <bool STREAM>
__device__ __forceinline__ void gb_spmm(const int32_t* rowptr, const int32_t* adj, const double* blocks, const double* x, const double* z, double* y,
                                        double* stage, int n, double alpha, double s1, double s2) {
    if (STREAM) {
        const double2* src = reinterpret_cast<const double2*>(x);
        for (int i = threadIdx.x; i < 3 * (BW / 2) * n; i += 256) { const double2 d = src[i]; stage[2 * i] = d.x; stage[2 * i + 1] = d.y; }
        __syncthreads();
        x = stage;
    }
    for (int i = threadIdx.x; i < BW * n; i += 256) {
        const int v = i / BW, c = i - v * BW;
        double acc[3] = {0.0, 0.0, 0.0};
        const int t1 = rowptr[v + 1];
        for (int t = rowptr[v]; t < t1; ++t) {
            double B[9];                                                 // column-major 3x3: B(r,k) = B[r + 3k]
            load_block9(blocks + 9 * (int64_t)t, B);
            const double* xu = x + 3 * BW * adj[t] + c;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double xv = xu[k * BW];
#pragma unroll
                for (int r = 0; r < 3; ++r) acc[r] += B[r + 3 * k] * xv;
            }
        }
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const int o = (3 * v + r) * BW + c;
            y[o] = alpha * acc[r] + s1 * x[o] + (s2 != 0.0 ? s2 * z[o] : 0.0);
        }
    }
    __syncthreads();
}

// G1 = X'Y (BOTH only), G2 = Y'Y over the 3n rows; results in LDS.  Ends with a barrier.
template <bool BOTH>
__device__ __forceinline__ void gb_gram(const double* X, const double* Y, int rows, double* G1, double* G2, double* red) {
    double g1[BW][BW], g2[BW][BW];
#pragma unroll
    for (int a = 0; a < BW; ++a)
#pragma unroll
        for (int b = 0; b < BW; ++b) { g1[a][b] = 0.0; g2[a][b] = 0.0; }
    for (int r = threadIdx.x; r < rows; r += 256) {
        double xr[BW], yr[BW];
#pragma unroll
        for (int c = 0; c < BW; ++c) { xr[c] = BOTH ? X[r * BW + c] : 0.0; yr[c] = Y[r * BW + c]; }
#pragma unroll
        for (int a = 0; a < BW; ++a)
#pragma unroll
            for (int b = 0; b < BW; ++b) { if (BOTH) g1[a][b] += xr[a] * yr[b]; g2[a][b] += yr[a] * yr[b]; }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < BW; ++a)
#pragma unroll
        for (int b = 0; b < BW; ++b) {
            const double s2 = group_sum<64>(g2[a][b]);
            if (lane == 0) red[wv * 2 * BW * BW + BW * BW + a * BW + b] = s2;
            if (BOTH) { const double s1 = group_sum<64>(g1[a][b]); if (lane == 0) red[wv * 2 * BW * BW + a * BW + b] = s1; }
        }
    __syncthreads();
    const int t = threadIdx.x;
    if (t < 2 * BW * BW && (BOTH || t >= BW * BW)) {
        const double tot = ((red[t] + red[2 * BW * BW + t]) + red[4 * BW * BW + t]) + red[6 * BW * BW + t];
        if (t < BW * BW) G1[t] = tot; else G2[t - BW * BW] = tot;
    }
    __syncthreads();
}

// Xn = Y * C over the 3n rows (C: BW x BW row-major in LDS, NC columns of it).  dst row stride = NC.  Ends with a barrier when LDS_DST.
template <int NC>
__device__ __forceinline__ void gb_combine(const double* Y, double* dst, int rows, const double* C) {
    for (int r = threadIdx.x; r < rows; r += 256) {
        double yr[BW];
#pragma unroll
        for (int c = 0; c < BW; ++c) yr[c] = Y[r * BW + c];
#pragma unroll
        for (int b = 0; b < NC; ++b) {
            double s = 0.0;
#pragma unroll
            for (int a = 0; a < BW; ++a) s += yr[a] * C[a * BW + b];
            dst[r * NC + b] = s;
        }
    }
    __syncthreads();
}

// max relative residual of the three wanted Ritz pairs: |Y z_c - theta_c X z_c| / max(|theta_1|, sigma); the same value in every thread
__device__ __forceinline__ double gb_residual(const double* X, const double* Y, int rows, const double* Z, const double* theta, double sigma, double* red) {
    double acc[3] = {0.0, 0.0, 0.0};
    for (int r = threadIdx.x; r < rows; r += 256) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            double yz = 0.0, xz = 0.0;
#pragma unroll
            for (int k = 0; k < BW; ++k) { yz += Y[r * BW + k] * Z[k * BW + c]; xz += X[r * BW + k] * Z[k * BW + c]; }
            const double d = yz - theta[c] * xz;
            acc[c] += d * d;
        }
    }
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int c = 0; c < 3; ++c) { const double s = group_sum<64>(acc[c]); if (lane == 0) red[wv * 3 + c] = s; }
    __syncthreads();
    double res = 0.0;
    const double scale = fmax(fabs(theta[0]), sigma);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const double r2 = ((red[c] + red[3 + c]) + red[6 + c]) + red[9 + c];
        res = fmax(res, sqrt(r2) / fmax(scale, 1e-300));
    }
    __syncthreads();                                                     // red is free again
    return res;
}

__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }

template <bool STREAM>
__global__ __launch_bounds__(256, 2) void k_gcw_batch(GbArgs a) {
    extern __shared__ double gb_lds[];
    const int b = a.list ? a.list[blockIdx.x] : (int)blockIdx.x, tid = threadIdx.x;
    const PbProb pd = a.prob[b];
    const int n = pd.n, m = pd.m, rows = 3 * n;
    const int32_t* rowptr = a.rowptr + pd.node_off + b;
    const int32_t* adj = a.adj + 2 * pd.edge_off;
    const int32_t* adj_eid = a.adj_eid + 2 * pd.edge_off;
    const double* rij = a.rij + 9 * pd.edge_off;
    double* blocks = a.blocks + 18 * pd.edge_off;
    double* dinv = a.dinv + pd.node_off;
    // LDS: four blocks of 18 n doubles, then G1[36] G2[36] Z[36] C[36] theta[6] red[288] ctl[10] = GB_SCRATCH
    // STREAM: the four blocks in the problem's workspace; LDS: the staging block of 18 n doubles, then the same small matrices
    double* X = STREAM ? a.work + 4 * 3 * BW * pd.node_off : gb_lds;
    double* Y = X + 3 * BW * n;
    double* P = Y + 3 * BW * n;
    double* Q = P + 3 * BW * n;
    double* stage = STREAM ? gb_lds : nullptr;
    double* G1 = STREAM ? gb_lds + 3 * BW * n : Q + 3 * BW * n;
    double* G2 = G1 + BW * BW;
    double* Z = G2 + BW * BW;
    double* Cm = Z + BW * BW;
    double* theta = Cm + BW * BW;
    double* red = theta + BW;
    double* ctl = red + 4 * 2 * BW * BW;
    double* Ident = P;                                                   // the identity for the start basis: P is free until the first filter

    // ---- weights (GCW.m:20), weighted degrees (GCW.m:21), D^-1/2
    const double* w = a.wts_in ? a.wts_in + pd.edge_off : nullptr;
    if (a.s_vec) {
        double* wo = a.w + pd.edge_off;
        for (int e = tid; e < m; e += 256) wo[e] = 1.0 / (pow(a.s_vec[pd.edge_off + e], 1.5) + 1e-8);
        w = wo;
        __syncthreads();
    }
    for (int v = tid; v < n; v += 256) {
        double acc = 0.0;
        for (int t = rowptr[v]; t < rowptr[v + 1]; ++t) acc += w ? w[adj_eid[t]] : 1.0;      // CSR order = the edge order of the problem
        X[v] = acc;
        dinv[v] = a.normalize ? (acc > 0 ? 1.0 / sqrt(acc) : 0.0) : 1.0;
    }
    __syncthreads();
    if (tid == 0) {
        double sg = 0.0;
        if (a.normalize) sg = 1.0;                                       // spectrum of D^-1/2 A D^-1/2 lies in [-1,1]
        else for (int v = 0; v < n; ++v) sg = fmax(sg, X[v]);           // ||A||_2 <= max weighted degree (orthogonal blocks)
        ctl[0] = sg;
    }
    // ---- blocks: slot t of row v = w_e dinv_v dinv_u (v < u ? R_e : R_e'); a wave per row, lanes over its slots
    {
        const int lane = tid & 63, wv = tid >> 6;
        for (int v = wv; v < n; v += 4) {
            const double dv = dinv[v];
            for (int t = rowptr[v] + lane; t < rowptr[v + 1]; t += 64) {
                const int u = adj[t], e = adj_eid[t];
                const double du = dinv[u];
                const double wt = (w ? w[e] : 1.0) * (v < u ? dv : du) * (v < u ? du : dv);  // same rounding in (v,u) and (u,v): exactly symmetric
                const double* R = rij + 9 * (int64_t)e;
                double* o = blocks + 9 * (int64_t)t;
                if (v < u) { for (int q = 0; q < 9; ++q) o[q] = wt * R[q]; }
                else { for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) o[r + 3 * c] = wt * R[c + 3 * r]; }
            }
        }
    }
    // ---- start block: hashed pseudo-random entries in [-1,1), t counted inside the problem
    for (int t = tid; t < rows * BW; t += 256) Y[t] = (double)(int64_t)(d_mix64(0xC0FFEEull + (uint64_t)t) >> 11) / 4503599627370496.0 - 1.0;
    if (tid < BW * BW) Ident[tid] = (tid % (BW + 1) == 0);
    __syncthreads();                                                     // dinv, blocks, ctl[0], Y and Ident are written
    const double sigma = ctl[0];
    double tol = a.tol;
    if (tol <= 0) tol = 1e-13;
    const int max_iters = a.max_iters <= 0 ? 500 : a.max_iters;

    int it = 0, products = 0, converged = 0, status = 0;
    double res = 1e300;
    // X = orth(X0)
    gb_gram<false>(Y, Y, rows, G1, G2, red);
    if (tid == 0) ctl[1] = ortho_coeffs<BW>(G2, Ident, Cm) ? 1.0 : 0.0;
    __syncthreads();
    if (uni(ctl[1] == 0.0)) status = 1;
    if (!status) {
        gb_combine<BW>(Y, X, rows, Cm);
        // Chebyshev-filtered subspace iteration: the tight scheme of spectral_impl (lo follows the block's own Ritz values, the degree of
        // a pass is what takes the residual to 0.2 tol, capped at 1e6 amplification and at 16)
        constexpr int CHEB_DEG = 16, CHEB_MIN = 2, CHEB_FIRST = 8;
        bool tight_ok = true;
        int cheb_deg = CHEB_FIRST;
        double res_prev = -1.0;
        double lo = -sigma, cut = 0.0;
        for (it = 1; it <= max_iters; ++it) {
            // ---- Rayleigh-Ritz on the current orthonormal basis X
            gb_spmm<STREAM>(rowptr, adj, blocks, X, X, Y, stage, n, 1.0, 0.0, 0.0); ++products;             // Y = A X
            gb_gram<true>(X, Y, rows, G1, G2, red);                                           // G1 = X'AX, G2 = Y'Y
            if (tid == 0) jacobi_eig<BW>(G1, theta, Z);
            __syncthreads();
            res = gb_residual(X, Y, rows, Z, theta, sigma, red);
            if (uni(res <= tol)) { converged = 1; break; }

            // ---- filter: P <- p(A) X with p small on [lo, cut], large above
            cut = theta[BW - 1];
            const double top = theta[0];
            if (tight_ok && it >= 2) {
                if (theta[BW - 1] <= lo || (res_prev > 0.0 && res > res_prev)) { lo = -sigma; tight_ok = false; }     // drifting to the negative end: the safe bound
                else lo = fmax(-sigma, -fmax(2.0 * fmax(fabs(theta[3]), fabs(theta[BW - 1])), 0.02 * sigma));
            }
            if (!(cut > lo) || !(top > cut)) cut = lo + 0.5 * (top - lo);                     // degenerate block: fall back to a mild filter
            const double e = 0.5 * (cut - lo), c = 0.5 * (cut + lo);
            if (it >= 2) {
                const double xi3 = (theta[2] - c) / e;
                cheb_deg = CHEB_DEG;
                if (xi3 > 1.0 + 1e-6 && res > 0.0) {
                    const double want = acosh(fmax(2.0, res / (0.2 * tol))), cap = acosh(1e6);
                    cheb_deg = (int)fmax((double)CHEB_MIN, fmin((double)CHEB_DEG, ceil(fmin(want, cap) / acosh(xi3))));
                }
            }
            cheb_deg = uni(cheb_deg);
            res_prev = res;
            double s_prev = e / (top - c);
            const double s1c = s_prev;
            gb_spmm<STREAM>(rowptr, adj, blocks, X, X, P, stage, n, s_prev / e, -c * s_prev / e, 0.0); ++products;   // P = (A X - c X) * s_prev / e
            double *Xp = X, *Pp = P, *Qp = Q;                                                 // X_{k-1}, X_k, scratch
            for (int k = 2; k <= cheb_deg; ++k) {
                const double s_new = 1.0 / (2.0 / s1c - s_prev);
                // Q = (2 s_new / e) (A P - c P) - (s_prev s_new) X_{k-1}
                gb_spmm<STREAM>(rowptr, adj, blocks, Pp, Xp, Qp, stage, n, 2.0 * s_new / e, -2.0 * s_new * c / e, -s_prev * s_new); ++products;
                double* t3 = Xp; Xp = Pp; Pp = Qp; Qp = t3;
                s_prev = s_new;
            }
            // ---- X <- orth(filtered block): into the buffer that held X_{k-1}; the three names are dealt again
            gb_gram<false>(Pp, Pp, rows, G1, G2, red);
            if (tid < BW * BW) Y[tid] = (tid % (BW + 1) == 0);                                // the identity: Y is free until the next product
            __syncthreads();
            if (tid == 0) ctl[1] = ortho_coeffs<BW>(G2, Y, Cm) ? 1.0 : 0.0;
            __syncthreads();
            if (uni(ctl[1] == 0.0)) { status = 2; break; }
            gb_combine<BW>(Pp, Xp, rows, Cm);
            X = Xp; P = Pp; Q = Qp;
        }
        if (!status) {
            // Z belongs to the basis in X in both exits (the loop leaves right after a Rayleigh-Ritz, or after max_iters with the last
            // Ritz rotation still unapplied: redo RR once)
            if (!converged && it > max_iters) {
                gb_spmm<STREAM>(rowptr, adj, blocks, X, X, Y, stage, n, 1.0, 0.0, 0.0); ++products;
                gb_gram<true>(X, Y, rows, G1, G2, red);
                if (tid == 0) jacobi_eig<BW>(G1, theta, Z);
                __syncthreads();
            }
            gb_combine<3>(X, a.V + 9 * pd.node_off, rows, Z);                                 // Ritz vectors V = X Z, the three wanted columns
        }
    }
    if (tid == 0) {
        GbInfo o;
        o.iters = it < max_iters ? it : max_iters; o.products = products; o.converged = converged; o.status = status; o.residual = res;
        for (int c = 0; c < 3; ++c) o.eig[c] = status ? 0.0 : theta[c];
        a.info[b] = o;
    }
}

}  // namespace
}  // namespace desc

namespace desc {

namespace {
// the refusals and the offsets; ii and jj sized, not filled
int batch_offsets_core(const desc_problem* probs, int32_t count, const std::function<int(int32_t, const desc_problem&)>& extra, BatchCsr* h,
                       bool allow_empty, bool need_rij = true) {
    h->count = count;
    h->node_off.assign((size_t)count + 1, 0); h->edge_off.assign((size_t)count + 1, 0);
    for (int32_t b = 0; b < count; ++b) {
        int rc = validate_problem(&probs[b], need_rij);
        if (rc) { const std::string msg = desc_last_error(); return fail(rc, "problem %d: %s", b, msg.c_str()); }
        if (probs[b].m == 0 && !allow_empty) return fail(DESC_ERR_INVALID, "problem %d: empty edge list", b);
        if (extra && (rc = extra(b, probs[b]))) return rc;
        h->node_off[(size_t)b + 1] = h->node_off[(size_t)b] + probs[b].n;
        h->edge_off[(size_t)b + 1] = h->edge_off[(size_t)b] + probs[b].m;
        h->max_n = std::max<int32_t>(h->max_n, (int32_t)probs[b].n);
    }
    h->N = h->node_off[(size_t)count]; h->M = h->edge_off[(size_t)count];
    if (h->M >= (1ll << 30))
        return fail(DESC_ERR_TOO_LARGE, "the batch holds %lld edges in total: the 2^30 index budget is exceeded, split the batch", (long long)h->M);
    h->ii.resize((size_t)h->M); h->jj.resize((size_t)h->M);
    return DESC_OK;
}
}  // namespace

int batch_offsets_host(const desc_problem* probs, int32_t count, const std::function<int(int32_t, const desc_problem&)>& extra, BatchCsr* h,
                       bool allow_empty, bool need_rij) {
    const int rc = batch_offsets_core(probs, count, extra, h, allow_empty, need_rij);
    if (rc) return rc;
    for_each_problem(count, [&](int32_t b) {
        const int64_t m = probs[b].m, eo = h->edge_off[(size_t)b];
        std::memcpy(h->ii.data() + eo, probs[b].ind_i, sizeof(int32_t) * (size_t)m);
        std::memcpy(h->jj.data() + eo, probs[b].ind_j, sizeof(int32_t) * (size_t)m);
    });
    return DESC_OK;
}

int batch_csr_host(const desc_problem* probs, int32_t count, const std::function<int(int32_t, const desc_problem&)>& extra, BatchCsr* h,
                   bool allow_empty) {
    const int rc = batch_offsets_core(probs, count, extra, h, allow_empty);
    if (rc) return rc;
    h->rowptr.resize((size_t)h->N + (size_t)count); h->adj.resize(2 * (size_t)h->M); h->adj_eid.resize(2 * (size_t)h->M);
    for_each_problem(count, [&](int32_t b) {
        hvec<int32_t> rp, ad, ae;
        const int64_t n = probs[b].n, m = probs[b].m, eo = h->edge_off[(size_t)b];
        std::memcpy(h->ii.data() + eo, probs[b].ind_i, sizeof(int32_t) * (size_t)m);
        std::memcpy(h->jj.data() + eo, probs[b].ind_j, sizeof(int32_t) * (size_t)m);
        build_csr(n, m, probs[b].ind_i, probs[b].ind_j, rp, ad, ae);
        std::memcpy(h->rowptr.data() + h->node_off[(size_t)b] + b, rp.data(), sizeof(int32_t) * (size_t)(n + 1));
        std::memcpy(h->adj.data() + 2 * eo, ad.data(), sizeof(int32_t) * 2 * (size_t)m);
        std::memcpy(h->adj_eid.data() + 2 * eo, ae.data(), sizeof(int32_t) * 2 * (size_t)m);
    });
    return DESC_OK;
}

}  // namespace desc

using namespace desc;

struct desc_gcw_batch : desc::BatchCsr, desc::BatchDevice {     // the set's offsets and endpoints; device, stream, arena, events
    const PbProb* d_prob = nullptr;
    const int32_t *d_rowptr = nullptr, *d_adj = nullptr, *d_adj_eid = nullptr;
    const double* d_rij = nullptr;
    double *d_in = nullptr, *d_w = nullptr, *d_dinv = nullptr, *d_blocks = nullptr, *d_V = nullptr;
    GbInfo* d_info = nullptr;
    // which kernel solves which problem (a function of the problem's own n and the mode alone); the lists are uploaded only where both run
    int32_t eig = DESC_GCW_EIG_LDS;
    std::vector<int32_t> lds_list, streamed_list;
    int32_t max_n_lds = 0, max_n_streamed = 0;
    int32_t *d_lds_list = nullptr, *d_streamed_list = nullptr;
    double* d_work = nullptr;
    std::shared_ptr<desc::PbSet> set;         // the owner of d_prob, the CSR and d_rij
    bool own_set = false;                     // the handle made the set from a problem list and is its only owner
    ~desc_gcw_batch() { close(); }            // the stream drains before the set may go
};

namespace {

int gb_check_eig(int32_t eig) {
    if (eig != DESC_GCW_EIG_LDS && eig != DESC_GCW_EIG_STREAMED && eig != DESC_GCW_EIG_AUTO)
        return fail(DESC_ERR_INVALID, "eig = %d is none of DESC_GCW_EIG_LDS (0), DESC_GCW_EIG_STREAMED (1), DESC_GCW_EIG_AUTO (2)", eig);
    return DESC_OK;
}

// the caps of the two kernels for problem b of n nodes
int gb_check_n(int32_t eig, int32_t b, int64_t n) {
    if (eig == DESC_GCW_EIG_LDS && n > GCW_BATCH_MAX_N)
        return fail(DESC_ERR_INVALID, "problem %d: n = %lld exceeds %d (the 3n x 6 blocks of the eigen-solve must fit the LDS of one workgroup): solve it with GCW / DESC_init",
                    b, (long long)n, GCW_BATCH_MAX_N);
    if (n > GCW_BATCH_STREAMED_MAX_N)
        return fail(DESC_ERR_INVALID, "problem %d: n = %lld exceeds %d (one 3n x 6 block of the streamed eigen-solve must fit the LDS of one workgroup): solve it with GCW / DESC_init",
                    b, (long long)n, GCW_BATCH_STREAMED_MAX_N);
    return DESC_OK;
}

// which kernel solves which problem, from the offsets
void gb_split(desc_gcw_batch* h) {
    for (int32_t b = 0; b < h->count; ++b) {
        const int32_t n = (int32_t)(h->node_off[(size_t)b + 1] - h->node_off[(size_t)b]);
        const bool streamed = h->eig == DESC_GCW_EIG_STREAMED || (h->eig == DESC_GCW_EIG_AUTO && n > GCW_BATCH_MAX_N);
        (streamed ? h->streamed_list : h->lds_list).push_back(b);
        int32_t& mx = streamed ? h->max_n_streamed : h->max_n_lds;
        mx = std::max(mx, n);
    }
}

// the run's own buffers
int gb_alloc_work(desc_gcw_batch* h) {
    const size_t M = (size_t)h->M, N = (size_t)h->N;
    int rc;
    if ((rc = h->mem.alloc(&h->d_in, M)) || (rc = h->mem.alloc(&h->d_w, M)) || (rc = h->mem.alloc(&h->d_dinv, N)) ||
        (rc = h->mem.alloc(&h->d_blocks, 18 * M)) || (rc = h->mem.alloc(&h->d_V, 9 * N)) || (rc = h->mem.alloc(&h->d_info, (size_t)h->count))) return rc;
    if (!h->streamed_list.empty()) {
        if ((rc = h->mem.alloc(&h->d_work, 4 * 3 * BW * N))) return rc;
        if (!h->lds_list.empty() &&
            ((rc = h->upload(&h->d_lds_list, h->lds_list.data(), h->lds_list.size())) ||
             (rc = h->upload(&h->d_streamed_list, h->streamed_list.data(), h->streamed_list.size())))) return rc;
    }
    return DESC_OK;
}

// The one create body, on a resident set: the caller's (desc_gcw_batch_create_on, probs = NULL), or one the handle makes from probs and
// owns alone (the list path; the cap is then refused per problem inside the set's host part, between the other refusals of that
// problem).  The handle adds nothing but the run's buffers: d_prob, the CSR and the rotations are the set's.
int gb_create(const desc_problem* probs, int32_t count, int32_t device, std::shared_ptr<PbSet> set, int32_t eig, desc_gcw_batch* h) {
    auto t0 = std::chrono::steady_clock::now();
    int rc = gb_check_eig(eig);
    if (rc) return rc;
    h->eig = eig;
    h->own_set = !set;
    if (h->own_set) {
        set = std::make_shared<PbSet>();
        rc = pb_host_part(probs, count, DESC_BUILD_HOST, [eig](int32_t b, const desc_problem& q) -> int { return gb_check_n(eig, b, q.n); }, set.get());
        if (rc) return rc;
    } else {
        for (int32_t b = 0; b < set->count; ++b)
            if ((rc = gb_check_n(eig, b, set->node_off[(size_t)b + 1] - set->node_off[(size_t)b]))) return rc;
    }
    h->set = set;
    pb_share_host(*set, h, !h->own_set);             // an own set: h->ii / h->jj stay EMPTY until pb_take_endpoints below -- read set->ii / set->jj till then
    gb_split(h);
    h->ms_structure = ms_since(t0);
    if (h->count == 0) return DESC_OK;

    const char* what = "the batched eigen-solve";
    if (h->own_set) {                                  // nothing above touched the device
        if ((rc = pb_device_part(probs, device, what, set.get()))) return rc;
        pb_take_endpoints(*set, h);
    }
    if ((rc = h->open(set->device, what))) return rc;
    auto t1 = std::chrono::steady_clock::now();
    h->d_prob = set->d_prob; h->d_rowptr = set->d_rowptr; h->d_adj = set->d_adj; h->d_adj_eid = set->d_adj_eid; h->d_rij = set->d_rij;
    if ((rc = gb_alloc_work(h))) return rc;
    DESC_HIP(hipStreamSynchronize(h->stream));         // the two lists may be on their way
    h->ms_upload = ms_since(t1) + (h->own_set ? set->ms_upload : 0);
    return DESC_OK;
}

int gb_run(desc_gcw_batch* h, const double* s_vec, const double* weights, int32_t normalize_rows, double tol, int32_t max_iters, double* R_out,
           desc_spectral_info* infos, desc_gcw_batch_timings* tm) {
    auto t0 = std::chrono::steady_clock::now();
    const int32_t count = h->count;
    if (tm) { tm->ms_structure = h->ms_structure; tm->ms_upload = h->ms_upload; tm->ms_eig = 0; tm->ms_project = 0; tm->ms_total = 0; }
    if (count == 0) { if (tm) tm->ms_total = ms_since(t0); return DESC_OK; }
    if (!R_out || !infos) return fail(DESC_ERR_INVALID, "R_out or infos is NULL");
    if (s_vec && weights) return fail(DESC_ERR_INVALID, "s_vec and weights are both set: pass one of them");
    const double* in = s_vec ? s_vec : weights;
    int rc;
    for (int32_t b = 0; b < count; ++b) {
        if (s_vec && (rc = check_s_vec_nonneg(*h, b, s_vec))) return rc;
        if (weights)
            for (int64_t e = h->edge_off[(size_t)b]; e < h->edge_off[(size_t)b + 1]; ++e)
                if (!(weights[e] >= 0) || !std::isfinite(weights[e]))
                    return fail(DESC_ERR_INVALID, "problem %d: weight %lld is not a finite non-negative number", b, (long long)(e - h->edge_off[(size_t)b]));
    }
    DESC_HIP(hipSetDevice(h->device));
    const size_t M = (size_t)h->M, N = (size_t)h->N;
    if (in) DESC_HIP(hipMemcpyAsync(h->d_in, in, sizeof(double) * M, hipMemcpyHostToDevice, h->stream));
    GbArgs a{};
    a.prob = h->d_prob; a.rowptr = h->d_rowptr; a.adj = h->d_adj; a.adj_eid = h->d_adj_eid; a.rij = h->d_rij;
    a.s_vec = s_vec ? h->d_in : nullptr; a.wts_in = weights ? h->d_in : nullptr;
    a.w = h->d_w; a.dinv = h->d_dinv; a.blocks = h->d_blocks; a.V = h->d_V; a.info = h->d_info;
    a.tol = tol; a.normalize = (s_vec || normalize_rows) ? 1 : 0; a.max_iters = max_iters;
    a.work = h->d_work;
    // at most two launches, each sized from the largest problem it solves; one kernel for the whole batch needs no list
    const size_t n_lds = h->lds_list.size(), n_streamed = h->streamed_list.size();
    const size_t lds = n_lds ? gb_lds_bytes(h->max_n_lds) : 0, lds_streamed = n_streamed ? gb_streamed_lds_bytes(h->max_n_streamed) : 0;
    if (std::max(lds, lds_streamed) > (size_t)GB_LDS_BYTES) return fail(DESC_ERR_STATE, "LDS budget exceeded (%zu bytes)", std::max(lds, lds_streamed));
    if (lds > 64 * 1024) DESC_HIP(hipFuncSetAttribute((const void*)k_gcw_batch<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    if (lds_streamed > 64 * 1024)
        DESC_HIP(hipFuncSetAttribute((const void*)k_gcw_batch<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds_streamed));
    if ((rc = h->timer_begin())) return rc;
    if (n_lds) {
        a.list = n_streamed ? h->d_lds_list : nullptr;
        hipLaunchKernelGGL(k_gcw_batch<false>, dim3((unsigned)n_lds), dim3(256), lds, h->stream, a);
        DESC_HIP(hipGetLastError());
    }
    if (n_streamed) {
        a.list = n_lds ? h->d_streamed_list : nullptr;
        hipLaunchKernelGGL(k_gcw_batch<true>, dim3((unsigned)n_streamed), dim3(256), lds_streamed, h->stream, a);
        DESC_HIP(hipGetLastError());
    }
    if ((rc = h->timer_end())) return rc;
    hvec<GbInfo> inf((size_t)count);
    hvec<double> V(9 * N), dinv(N);
    DESC_HIP(hipMemcpyAsync(inf.data(), h->d_info, sizeof(GbInfo) * (size_t)count, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipMemcpyAsync(V.data(), h->d_V, sizeof(double) * 9 * N, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipMemcpyAsync(dinv.data(), h->d_dinv, sizeof(double) * N, hipMemcpyDeviceToHost, h->stream));
    DESC_HIP(hipStreamSynchronize(h->stream));
    float ms = 0;
    if ((rc = h->timer_ms(&ms))) return rc;
    for (int32_t b = 0; b < count; ++b) {
        if (inf[(size_t)b].status == 1) return fail(DESC_ERR_INVALID, "problem %d: degenerate start basis", b);
        if (inf[(size_t)b].status) return fail(DESC_ERR_INVALID, "problem %d: subspace iteration broke down (rank-deficient block)", b);
    }
    // ---- the tail of spectral_impl per problem on host threads
    auto t1 = std::chrono::steady_clock::now();
    for_each_problem(count, [&](int32_t b) {
        const int64_t no = h->node_off[(size_t)b], n = h->node_off[(size_t)b + 1] - no;
        double* Vb = V.data() + 9 * (size_t)no;
        ritz_scale_sign(Vb, a.normalize ? dinv.data() + no : nullptr, n);
        project_nodes(Vb, 0, n, R_out + 9 * (size_t)no);
    });
    const double ms_project = ms_since(t1), ms_total = ms_since(t0);
    for (int32_t b : h->streamed_list) infos[b].reserved = 1;
    for (int32_t b : h->lds_list) infos[b].reserved = 0;
    for (int32_t b = 0; b < count; ++b) {
        const GbInfo& g = inf[(size_t)b];
        desc_spectral_info& o = infos[b];
        o.iters = g.iters; o.products = g.products; o.converged = g.converged; o.residual = g.residual;
        for (int c = 0; c < 3; ++c) o.eigenvalues[c] = g.eig[c];
        o.ms_total = ms_total;
    }
    if (tm) { tm->ms_eig = ms; tm->ms_project = ms_project; tm->ms_total = ms_total; }
    return DESC_OK;
}

}  // namespace

extern "C" {

int32_t desc_gcw_batch_max_n(void) { return GCW_BATCH_MAX_N; }

int32_t desc_gcw_batch_streamed_max_n(void) { return GCW_BATCH_STREAMED_MAX_N; }

int desc_gcw_batch_create(const desc_problem* probs, int32_t count, int32_t device, desc_gcw_batch** out) {
    return batch_create_guarded("desc_gcw_batch_create", out, probs, count,
                                [&](desc_gcw_batch* h) { return gb_create(probs, count, device, nullptr, DESC_GCW_EIG_LDS, h); });
}

int desc_gcw_batch_create_where(const desc_problem* probs, int32_t count, int32_t device, int32_t eig, desc_gcw_batch** out) {
    return batch_create_guarded("desc_gcw_batch_create_where", out, probs, count,
                                [&](desc_gcw_batch* h) { return gb_create(probs, count, device, nullptr, eig, h); });
}

int desc_gcw_batch_create_on(desc_problem_batch* set, int32_t eig, desc_gcw_batch** out) {
    return batch_create_guarded("desc_gcw_batch_create_on", out, set, 0, [&](desc_gcw_batch* h) { return gb_create(nullptr, 0, 0, set->s, eig, h); }, set != nullptr);
}

int desc_gcw_batch_bytes(const desc_gcw_batch* h, int64_t* h2d, int64_t* d2h) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    return batch_bytes_on_set(*h, h->own_set ? h->set.get() : nullptr, h2d, d2h);
}

int desc_gcw_batch_sizes(const desc_gcw_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    return batch_sizes(*h, count, node_off, edge_off);
}

int desc_gcw_batch_csr(const desc_problem* probs, int32_t count, int64_t* node_off, int64_t* edge_off, int32_t* rowptr, int32_t* adj, int32_t* adj_eid) {
    return no_throw("desc_gcw_batch_csr", [&]() -> int {
        if (count < 0 || (count > 0 && !probs) || !node_off || !edge_off) return fail(DESC_ERR_INVALID, "NULL argument or negative count");
        BatchCsr h;
        int rc = batch_csr_host(probs, count, [](int32_t b, const desc_problem& q) -> int { return gb_check_n(DESC_GCW_EIG_LDS, b, q.n); }, &h);
        if (rc) return rc;
        batch_sizes(h, nullptr, node_off, edge_off);
        if (rowptr) std::copy(h.rowptr.begin(), h.rowptr.end(), rowptr);
        if (adj) std::copy(h.adj.begin(), h.adj.end(), adj);
        if (adj_eid) std::copy(h.adj_eid.begin(), h.adj_eid.end(), adj_eid);
        return DESC_OK;
    });
}

int desc_gcw_batch_run(desc_gcw_batch* h, const double* s_vec, const double* weights, int32_t normalize_rows, double tol, int32_t max_iters,
                       double* R_out, desc_spectral_info* infos, desc_gcw_batch_timings* timings) {
    return no_throw("desc_gcw_batch_run", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        return gb_run(h, s_vec, weights, normalize_rows, tol, max_iters, R_out, infos, timings);
    });
}

void desc_gcw_batch_destroy(desc_gcw_batch* h) { delete h; }

}  // extern "C"

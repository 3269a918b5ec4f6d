// Rotation_Alignment (Utils/Rotation_Alignment.m:13-38) for many problems in one GPU pass (desc_align_batch_*): the scoring behind the
// *_batch solvers of a Monte-Carlo study.  The operand orders stand in include/desc_amd.h; tests/align_batch_oracle.py restates the
// summation orders, the median rule and the projection in NumPy.
//
// The problems lie behind one another, as R_out of desc_gcw_batch_run: problem b's 3x3xn_b column-major blocks start at 9 * node_off[b].
//
//   k_align_batch   one workgroup of 256 threads per problem, blockIdx.x the problem
//     pass 1   :18-22  thread t takes the nodes t, t + 256, ...: the nine entries of R_est_k' R_gt_k into nine running sums; the 256
//                      partials by group_sum<64> inside a wave, then the waves 0..3 in order (as gb_gram of gcw_batch.hip)
//     R_align  :24-25  every thread projects the same A from LDS (mb_project of so3_blocks.h: svd3 of irls_math.h); thread 0 stores it
//     pass 2   :30-34  chunks of 256 nodes: R_out_k = R_est_k R_align, the trace with R_gt_k, the error in degrees to global memory; the
//                      R_out blocks through LDS, consecutive lanes to consecutive doubles (skipped where the caller wants no R_out).  The
//                      R_est and R_gt blocks are read again from L2: no per-node state lives in LDS, so LDS sets no cap on n
//     mean     :35     thread-strided partials in ascending node order, the same fixed reduction, / n
//     median   :36     MATLAB's median by the exact radix select of laa_wg.h (wg_select) over the errors in global memory: the order
//                      statistic of rank (n + 1) / 2, or a + (b - a) / 2 of the two middle ones
//   k_align_project the test hook: the projection alone, one thread per block
//
// Composition independence.  A problem's workgroup reads its own blocks and its own n; which workgroup runs it, and what else the batch
// holds, enters no result.
//
// Control flow (the rules at the top of laa_wg.h).  Every thread takes every barrier: the chunk loop of pass 2 and the selection are
// steered by n and by the R_out pointer, the same in all 256 threads, and n goes through readfirstlane.  Every loop is bounded by n or
// the 8 digit passes.  No spinning on memory, no floating-point atomic (the histogram of the selection counts in integers).
#include <chrono>
#include <cmath>
#include <new>

#include "batch_device.h"
#include "laa_wg.h"
#include "pgd_math.h"
#include "so3_blocks.h"

namespace desc {
namespace {

constexpr int64_t AB_MAX_NODES = ((1ll << 31) + 8) / 9;      // 9 N < 2^31: a block's first double is an int32 offset

struct AbArgs {
    const int32_t* node_off = nullptr;          // B + 1
    const double *r_gt = nullptr, *r_est = nullptr;           // N x 9
    double *r_out = nullptr;                    // N x 9; null: the caller wants no R_out
    double *r_align = nullptr, *err = nullptr, *mean = nullptr, *median = nullptr;      // B x 9, N, B, B
};

// the workgroup's sum of v: lanes by group_sum<64>, the waves 0..3 in order.  red: 4 doubles of LDS.  Starts and ends with a barrier.
__device__ __forceinline__ double ab_sum(double v, double* red) {
    const double s = group_sum<64>(v);
    __syncthreads();                                              // red's last readers are done
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

__global__ __launch_bounds__(256) void k_align_batch(AbArgs a) {
    __shared__ double red[4 * 9];
    __shared__ double stage[256 * 9];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int off = uniform_load(a.node_off, b);
    const int n = uni(uniform_load(a.node_off, b + 1) - off);
    const double* E = a.r_est + 9 * (int64_t)off;
    const double* G = a.r_gt + 9 * (int64_t)off;
    double* err = a.err + off;
    // ---- pass 1: A = sum_k R_est_k' R_gt_k (:18-22)
    double A[9];
    for (int q = 0; q < 9; ++q) A[q] = 0.0;
    for (int k = tid; k < n; k += 256) {
        double e[9], g[9];
        load_block9(E + 9 * (int64_t)k, e);
        load_block9(G + 9 * (int64_t)k, g);
        for (int c = 0; c < 3; ++c)
            for (int r = 0; r < 3; ++r) {
                double s = 0.0;
                for (int i = 0; i < 3; ++i) s += e[i + 3 * r] * g[i + 3 * c];
                A[r + 3 * c] += s;
            }
    }
    for (int q = 0; q < 9; ++q) { const double s = group_sum<64>(A[q]); if (lane == 0) red[wv * 9 + q] = s; }
    __syncthreads();
    for (int q = 0; q < 9; ++q) A[q] = ((red[q] + red[9 + q]) + red[18 + q]) + red[27 + q];
    // ---- R_align = U1 diag(1, 1, det(U1 V1')) V1' (:24-25): every thread, from the same LDS values
    double Ra[9];
    mb_project(A, Ra);
    if (tid == 0) for (int q = 0; q < 9; ++q) a.r_align[9 * (int64_t)b + q] = Ra[q];
    // ---- pass 2: R_out, the errors in degrees (:30-34)
    double esum = 0.0;
    for (int base = 0; base < n; base += 256) {
        const int k = base + tid;
        double o[9];
        for (int q = 0; q < 9; ++q) o[q] = 0.0;
        if (k < n) {
            double e[9], g[9];
            load_block9(E + 9 * (int64_t)k, e);
            load_block9(G + 9 * (int64_t)k, g);
            for (int c = 0; c < 3; ++c)
                for (int r = 0; r < 3; ++r) {
                    double s = 0.0;
                    for (int i = 0; i < 3; ++i) s += e[r + 3 * i] * Ra[i + 3 * c];
                    o[r + 3 * c] = s;
                }
            double tr = 0.0;
            for (int q = 0; q < 9; ++q) tr += g[q] * o[q];
            const double ek = abs_acos_ext((tr - 1.0) / 2.0) / M_PI * 180;
            err[k] = ek;
            esum += ek;
        }
        if (a.r_out) mb_store_blocks(stage, a.r_out + 9 * ((int64_t)off + base), o, min(256, n - base));
    }
    // ---- mean_error (:35)
    const double mean = ab_sum(esum, red) / (double)n;
    // ---- median_error (:36): the first barrier of wg_select orders the errors written above
    const int64_t k0 = (int64_t)((n - 1) >> 1);
    const bool even = (n & 1) == 0;
    unsigned long long klo = 0, khi = 0;
    double med = NAN;
    if (!wg_select(err, n, k0, even, &klo, &khi)) {
        const double lo = key_value(klo), hi = key_value(khi);
        med = even ? lo + (hi - lo) / 2.0 : lo;
    }
    if (tid == 0) { a.mean[b] = mean; a.median[b] = med; }
}

__global__ __launch_bounds__(256) void k_align_project(const double* A, int64_t count, double* R) {
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < count; t += (int64_t)gridDim.x * 256) {
        double q[9], r[9];
        load_block9(A + 9 * t, q);
        mb_project(q, r);
        for (int k = 0; k < 9; ++k) R[9 * t + k] = r[k];
    }
}

// the first non-finite entry of the problems' blocks: refusal naming the problem and the 1-based node
int ab_check_finite(const double* R, const hvec<int64_t>& node_off, int32_t count, const char* what) {
    for (int32_t b = 0; b < count; ++b)
        for (int64_t g = node_off[(size_t)b]; g < node_off[(size_t)b + 1]; ++g) {
            bool ok = true;
            for (int k = 0; k < 9; ++k) ok = ok && std::isfinite(R[9 * g + k]);
            if (!ok) return fail(DESC_ERR_INVALID, "problem %d: %s of node %lld is not finite", (int)b, what, (long long)(g - node_off[(size_t)b] + 1));
        }
    return DESC_OK;
}

}  // namespace
}  // namespace desc

using namespace desc;

struct desc_align_batch : BatchDevice {
    int32_t count = 0;
    int64_t N = 0;
    hvec<int64_t> node_off;
    AbArgs a;
    double* d_est = nullptr;
    double* d_out = nullptr;
};

namespace {

int ab_create(const int32_t* n, const double* R_gt, int32_t count, int32_t device, desc_align_batch* h) {
    h->count = count;
    h->node_off.assign((size_t)count + 1, 0);
    int64_t N = 0;
    for (int32_t b = 0; b < count; ++b) {
        if (n[b] < 1) return fail(DESC_ERR_INVALID, "problem %d: n = %d, need n >= 1", (int)b, (int)n[b]);
        N += n[b];
        if (N >= AB_MAX_NODES) return fail(DESC_ERR_TOO_LARGE, "the batch holds 2^31 / 9 nodes or more at problem %d: split the batch", (int)b);
        h->node_off[(size_t)b + 1] = N;
    }
    h->N = N;
    if (count == 0) return DESC_OK;
    int rc = ab_check_finite(R_gt, h->node_off, count, "R_gt");
    if (rc) return rc;

    if ((rc = h->open(device, "the batched rotation alignment"))) return rc;           // nothing above touched the device
    const size_t B = (size_t)count, Ns = (size_t)N;
    hvec<int32_t> off32(B + 1);
    for (size_t b = 0; b <= B; ++b) off32[b] = (int32_t)h->node_off[b];
    AbArgs& a = h->a;
    if ((rc = h->upload(&a.node_off, off32.data(), B + 1)) || (rc = h->upload(&a.r_gt, R_gt, 9 * Ns)) || (rc = h->mem.alloc(&h->d_est, 9 * Ns)) ||
        (rc = h->mem.alloc(&h->d_out, 9 * Ns)) || (rc = h->mem.alloc(&a.r_align, 9 * B)) || (rc = h->mem.alloc(&a.err, Ns)) ||
        (rc = h->mem.alloc(&a.mean, B)) || (rc = h->mem.alloc(&a.median, B))) return rc;
    a.r_est = h->d_est;
    DESC_HIP(hipStreamSynchronize(h->stream));                                          // off32 goes out of scope; R_gt is the caller's
    return DESC_OK;
}

}  // namespace

extern "C" {

int desc_align_batch_create(const int32_t* n, const double* R_gt, int32_t count, int32_t device, desc_align_batch** out) {
    return batch_create_guarded("desc_align_batch_create", out, n, count, [&](desc_align_batch* h) { return ab_create(n, R_gt, count, device, h); },
                                count <= 0 || R_gt != nullptr);
}

int desc_align_batch_sizes(const desc_align_batch* h, int32_t* count, int64_t* node_off) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    if (count) *count = h->count;
    if (node_off) for (int32_t b = 0; b <= h->count; ++b) node_off[b] = h->node_off[(size_t)b];
    return DESC_OK;
}

int desc_align_batch_run(desc_align_batch* h, const double* R_est, double* R_out, double* R_align, double* err, double* mean_error,
                         double* median_error, desc_align_batch_timings* tm) {
    return no_throw("desc_align_batch_run", [&]() -> int {
        if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
        auto t0 = std::chrono::steady_clock::now();
        if (tm) { tm->ms_upload = 0; tm->ms_align = 0; tm->ms_copy = 0; tm->ms_total = 0; }
        if (h->count == 0) return DESC_OK;
        if (!R_est || !R_align || !mean_error || !median_error) return fail(DESC_ERR_INVALID, "NULL argument");
        int rc = ab_check_finite(R_est, h->node_off, h->count, "R_est");
        if (rc) return rc;
        const size_t B = (size_t)h->count, N = (size_t)h->N;
        DESC_HIP(hipSetDevice(h->device));
        DESC_HIP(hipMemcpyAsync(h->d_est, R_est, sizeof(double) * 9 * N, hipMemcpyHostToDevice, h->stream));
        DESC_HIP(hipStreamSynchronize(h->stream));
        const double ms_upload = ms_since(t0);
        auto t1 = std::chrono::steady_clock::now();
        AbArgs a = h->a;
        a.r_out = R_out ? h->d_out : nullptr;
        hipLaunchKernelGGL(k_align_batch, dim3((unsigned)B), dim3(256), 0, h->stream, a);
        DESC_HIP(hipGetLastError());
        DESC_HIP(hipStreamSynchronize(h->stream));
        const double ms_align = ms_since(t1);
        auto t2 = std::chrono::steady_clock::now();
        if (R_out) DESC_HIP(hipMemcpyAsync(R_out, h->d_out, sizeof(double) * 9 * N, hipMemcpyDeviceToHost, h->stream));
        DESC_HIP(hipMemcpyAsync(R_align, a.r_align, sizeof(double) * 9 * B, hipMemcpyDeviceToHost, h->stream));
        if (err) DESC_HIP(hipMemcpyAsync(err, a.err, sizeof(double) * N, hipMemcpyDeviceToHost, h->stream));
        DESC_HIP(hipMemcpyAsync(mean_error, a.mean, sizeof(double) * B, hipMemcpyDeviceToHost, h->stream));
        DESC_HIP(hipMemcpyAsync(median_error, a.median, sizeof(double) * B, hipMemcpyDeviceToHost, h->stream));
        DESC_HIP(hipStreamSynchronize(h->stream));
        if (tm) { tm->ms_upload = ms_upload; tm->ms_align = ms_align; tm->ms_copy = ms_since(t2); tm->ms_total = ms_since(t0); }
        return DESC_OK;
    });
}

void desc_align_batch_destroy(desc_align_batch* h) { delete h; }

int desc_test_align_project(const double* A, int64_t count, int32_t device, double* R) {
    return no_throw("desc_test_align_project", [&]() -> int {
        if (!A || !R || count < 0) return fail(DESC_ERR_INVALID, "NULL argument or negative count");
        if (count == 0) return DESC_OK;
        BatchDevice dev;
        int rc = dev.open(device, "the alignment's projection hook");
        if (rc) return rc;
        const double* dA = nullptr;
        double* dR = nullptr;
        if ((rc = dev.upload(&dA, A, 9 * (size_t)count)) || (rc = dev.mem.alloc(&dR, 9 * (size_t)count))) return rc;
        hipLaunchKernelGGL(k_align_project, dim3((unsigned)grid_for(count, 4096)), dim3(256), 0, dev.stream, dA, count, dR);
        DESC_HIP(hipGetLastError());
        DESC_HIP(hipMemcpyAsync(R, dR, sizeof(double) * 9 * (size_t)count, hipMemcpyDeviceToHost, dev.stream));
        DESC_HIP(hipStreamSynchronize(dev.stream));
        return DESC_OK;
    });
}

}  // extern "C"

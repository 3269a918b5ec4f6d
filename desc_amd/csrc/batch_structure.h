// The batched device structure builder (batch_structure.hip) as batch.hip sees it, and the plan rule both sides of it share.
// Internal; the C ABI keeps desc_pgd_batch opaque.
#pragma once
#include "batch_csr.h"
#include "batch_device.h"
#include "cemp_batch.h"
#include "problem_batch.h"

namespace desc {

// What the cycle lists of one problem will look like, from the histogram of its codegrees alone (DESC_PGD.m:36-51).
struct BatchPlan {
    int64_t m_pos;            // edges with a 3-cycle
    int64_t m_cycle;          // sum of min(codeg, n_sample)
    int32_t max_codeg;
    int32_t n_sample;         // max(n_sample_min, ceil(median of the positive codegrees / 4)), MATLAB's median
    int32_t max_cnt;          // min(max_codeg, n_sample): the longest segment
    int32_t pad;
};

// hist[c] = number of edges with codegree c, c = 0 .. n (a codegree is at most n - 2).  The rule of the single device builder
// (structure_device.hip: "edges with cycles, median, n_sample, m_cycle"), in one pass per quantity over the n + 1 bins; run by the
// plan kernel (one record per problem) and, for the tests, by desc_test_batch_plan on the host.
__host__ __device__ inline void batch_plan_rule(const int32_t* hist, int32_t n, int32_t n_sample_min, BatchPlan* out) {
    int64_t mp = 0;
    int32_t max_codeg = 0;
    for (int32_t c = 1; c <= n; ++c) if (hist[c]) { mp += hist[c]; max_codeg = c; }
    int32_t n_sample = n_sample_min;                  // median([]) = NaN, max(NaN, 30) = 30
    if (mp > 0) {
        // the two middle values: the r-th smallest positive codegree (0-based) is the first c whose running count exceeds r
        const int64_t r_hi = mp / 2, r_lo = (mp & 1) ? mp / 2 : mp / 2 - 1;
        double lo = (double)max_codeg, hi = (double)max_codeg;
        bool have_lo = false;
        int64_t acc = 0;
        for (int32_t c = 1; c <= n; ++c) {
            acc += hist[c];
            if (!have_lo && acc > r_lo) { lo = (double)c; have_lo = true; }
            if (acc > r_hi) { hi = (double)c; break; }
        }
        const double med = (mp & 1) ? hi : 0.5 * (lo + hi);                    // MATLAB median (:43)
        const int32_t q = (int32_t)ceil(med / 4.0);
        n_sample = q > n_sample_min ? q : n_sample_min;
    }
    int64_t mc = 0;
    for (int32_t c = 1; c <= n; ++c) mc += (int64_t)hist[c] * (int64_t)(c < n_sample ? c : n_sample);      // :45-51
    out->m_pos = mp; out->m_cycle = mc; out->max_codeg = max_codeg; out->n_sample = n_sample;
    out->max_cnt = max_codeg < n_sample ? max_codeg : n_sample;
    out->pad = 0;
}

// Largest codegree the sampling kernel stages: per wave and staged common neighbour a key (8 B) and the packed row positions (4 B),
// 4 waves x 1024 x 12 B = 48 KiB of the 64 KiB a launch may declare.
constexpr int BATCH_MAX_CODEG = 1024;
static_assert(4 * BATCH_MAX_CODEG * (8 + 4) <= 64 * 1024, "LDS budget");
static_assert(BATCH_MAX_CODEG <= CEMP_BATCH_MAX_DEGREE, "a codegree is bounded by a CSR row");

constexpr int BATCH_BUILD_FALLBACK = 1;      // not an error: the batch is outside what the device builder stages, build it on the host
constexpr int BATCH_BUILD_LAPS = 5;          // codegrees, plan, compaction, sampling, mirror maps

// The index arrays of a PGD batch, made on the device (blocks of dev->mem, written on dev->stream, which has drained on return).
struct BatchBuilt {
    hvec<BatchPlan> plan;                      // per problem
    hvec<int64_t> edge_off, cycle_off, seg_off;
    int32_t *d_cum = nullptr, *d_pos = nullptr, *d_ejk = nullptr, *d_eki = nullptr, *d_ikj = nullptr, *d_jki = nullptr;
    int32_t *d_kk = nullptr, *d_codeg = nullptr;
    const int32_t *d_ii = nullptr, *d_jj = nullptr;    // the builder's own uploads, or the set's
    double ms_lap[BATCH_BUILD_LAPS] = {0, 0, 0, 0, 0};      // device time of the five launches (HIP events)
};

// validate -> batch_csr_host -> open(device) -> uploads -> codegrees, plan -> the one read-back -> refusals -> compaction, sampling,
// mirror maps.  Returns DESC_OK, an error code (the refusals of the host path, same code and same "problem b") or BATCH_BUILD_FALLBACK
// (a CSR row above CEMP_BATCH_MAX_DEGREE: before the device is opened; a codegree above BATCH_MAX_CODEG: after the read-back).
// set (nullable): a resident problem set the problems come from (problem_batch.h; probs then views its host endpoints and device is the
// set's).  Nothing is validated or laid out again, the edge list and the CSR are the set's device arrays, the edge -> problem map is
// filled by a launch, and the uploads of the build are O(B) bytes.
int batch_structure_device(BatchDevice* dev, const desc_problem* probs, int32_t count, int32_t n_sample_min, uint64_t seed,
                           const uint64_t* seeds, int32_t device, BatchBuilt* out, const PbSet* set = nullptr);

}  // namespace desc

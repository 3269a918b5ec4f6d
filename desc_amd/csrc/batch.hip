// DESC_PGD for many small problems in one GPU pass (desc_pgd_batch_*).
//
// The reference's users run Monte-Carlo studies: hundreds of graphs of 100-200 nodes.  One such graph leaves the card almost idle
// (a latency-bound chain of launches and stop-flag polls per call), so B of them are laid behind one another in ONE set of device
// arrays and every iteration is ONE sweep launch plus one bookkeeping launch for the whole batch.
//
// Layout.  The structures are built per problem by the host builder (local ids: bit-exact with a solve of the problem alone) and
// concatenated with per-problem edge / cycle offsets added (batch_concat) -- or, with desc_pgd_batch_create_where(DESC_BUILD_DEVICE),
// the same arrays, element for element, are made for the whole batch on the device (batch_structure.hip); batch_finish and the run
// see no difference.  The sweep is the gather sweep of sweep_gather.hip (k_sweep<G, STEP>):
// a group of G lanes per segment, mirror sums from direct gathers of w_old[ikj] / w_old[jki], tangent projection, plugin step, simplex
// projection, new S -- the arithmetic comes from pgd_math.h, shared with pgd.hip.
//
// Workgroup table.  Workgroup g sweeps segments seg0 .. seg0 + nseg of ONE problem with that problem's lane-group width; a problem's
// segments are cut into runs of 4 passes x 4 waves x 64/G segments counted from the problem's own first segment.  A workgroup returns at
// once when its problem's stop flag is set.
//
// Composition independence.  Everything that decides a bit of problem b's result depends on b alone: G (b's longest segment), the cut
// into workgroups (b's segment count), the lanes a segment lands on (its index inside b), the order of the workgroup partials in
// k_batch_finalize (b's own partials, lane v adds v, v + 64, ... and the fixed butterfly combines the lanes).  No atomics on doubles.
//
// Stop rule.  As in pgd.hip the objective of iterate t is accumulated by sweep t + 1 (which gathers exactly those values), so the
// patience rule for t is applied by the bookkeeping launch behind sweep t + 1.  When it fires for problem b, what sweep t + 1 wrote for
// b is discarded: w, S and the Adam moments are double-buffered, iterate t sits in the buffers of parity t & 1, which sweep t + 1 only
// read, and b's workgroups never run again.  The parity is recorded per problem; k_batch_settle brings every problem's final state
// into buffer 0 before the download.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <new>
#include <vector>

#include "batch_csr.h"
#include "batch_device.h"
#include "batch_structure.h"
#include "pgd_math.h"

namespace desc {
namespace {

constexpr int BATCH_PASSES = 4;      // passes of the 4 waves of a workgroup over its run of segments

struct BatchState {
    int32_t stop;          // 1 once the patience rule fired for this problem
    int32_t misses;        // DESC_PGD.m:181
    int32_t iters_run;     // iteration at which the loop broke
    int32_t final_parity;  // which double buffer holds the final iterate
};
struct BatchWg { int32_t prob, seg0, nseg, G; };
struct BatchProb { int32_t wg0, nwg; int64_t m; };     // workgroups of the problem, its edge count (average_change divides by it)

struct BatchArgs {
    const int32_t* cum;       // segments of the whole batch + 1 (global cycle positions)
    const int32_t* pos_edge;  // global edge ids
    const int32_t* e_jk;
    const int32_t* e_ki;
    const int32_t* ikj;
    const int32_t* jki;
    const double* S0;
    const double* w_old;
    double* w_new;
    const double* S_old;
    double* S_new;
    const double* nv_tab;     // nv_tab[c] = 1/sqrt(c), c <= 64 (DESC_PGD.m:199)
    double* partials;         // [workgroup][2]: objective of the old iterate, sum |dS|
    const BatchState* state;
    const BatchWg* wg;
    StepArgs st;
};

// the loop of k_sweep<G, STEP> (sweep_gather.hip) over the segments lo .. hi of one problem
template <int G, int STEP>
__device__ __forceinline__ void batch_sweep_run(const BatchArgs& a, int lo, int hi, double& obj_acc, double& chg_acc) {
    constexpr int EPW = 64 / G;
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int sub = lane / G, gl = lane % G;
    for (int l0 = lo + wv * EPW; l0 < hi; l0 += 4 * EPW) {
        const int l = l0 + sub;
        const bool edge_ok = l < hi;
        int base = 0, cnt = 0;
        if (edge_ok) { base = a.cum[l]; cnt = a.cum[l + 1] - base; }
        const bool act0 = gl < cnt;
        const int64_t c = (int64_t)base + gl;

        double w = 0.0, d = 0.0, ssum = 0.0, wa = 0.0, wb = 0.0;
        int ia = -1, ib = -1;
        if (act0) {
            const int ejk = a.e_jk[c], eki = a.e_ki[c];
            ia = a.ikj[c]; ib = a.jki[c];
            w = a.w_old[c]; d = a.S0[c];
            ssum = a.S_old[ejk] + a.S_old[eki];
            if (ia >= 0) wa = a.w_old[ia];
            if (ib >= 0) wb = a.w_old[ib];
        }
        obj_acc += w * ssum;                       // objective of the iterate being read (:233, one sweep late)
        // mirror-weight sums: one scalar per edge, applied to masked positions only (:189-190)
        const double T1 = group_sum<G>(wa), T2 = group_sum<G>(wb);
        double g = ssum + ((ia >= 0 ? T1 : 0.0) + (ib >= 0 ? T2 : 0.0)) * d;          // :193
        // tangent projection grad - (grad*nv')*nv, nv = ones/sqrt(cnt)  (:199-201)
        const double nv = act0 ? a.nv_tab[cnt] : 0.0;
        const double dot = group_sum<G>(act0 ? g * nv : 0.0);
        g = g - dot * nv;
        const double ws = act0 ? apply_step<STEP>(a.st, w, g, c) : 0.0;               // :207
        const double T = simplex_threshold<G>(ws, act0, lane);                        // :215-223
        const double wn = act0 ? fmax(ws - T, 0.0) : 0.0;                             // :224
        const double snew = group_sum<G>(wn * d);                                     // :229
        if (act0) a.w_new[c] = wn;
        if (edge_ok && gl == 0) {
            const int e = a.pos_edge[l];
            chg_acc += fabs(snew - a.S_old[e]);                                       // :232
            a.S_new[e] = snew;
        }
    }
}

// one pair of partials per workgroup: the 64 lanes of a wave by the fixed butterfly, the 4 waves in order
__device__ __forceinline__ void batch_block_partials(double obj_acc, double chg_acc, double* partials, int g) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    obj_acc = group_sum<64>(obj_acc);
    chg_acc = group_sum<64>(chg_acc);
    __shared__ double sh[8];
    if (lane == 0) { sh[wv] = obj_acc; sh[4 + wv] = chg_acc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        partials[2 * g] = ((sh[0] + sh[1]) + sh[2]) + sh[3];
        partials[2 * g + 1] = ((sh[4] + sh[5]) + sh[6]) + sh[7];
    }
}

template <int STEP>
__global__ __launch_bounds__(256) void k_batch_sweep(BatchArgs a) {
    const BatchWg g = a.wg[blockIdx.x];
    if (a.state[g.prob].stop) return;              // uniform over the workgroup: a stopped problem is frozen
    double obj_acc = 0.0, chg_acc = 0.0;
    if (g.G == 16) batch_sweep_run<16, STEP>(a, g.seg0, g.seg0 + g.nseg, obj_acc, chg_acc);
    else if (g.G == 32) batch_sweep_run<32, STEP>(a, g.seg0, g.seg0 + g.nseg, obj_acc, chg_acc);
    else batch_sweep_run<64, STEP>(a, g.seg0, g.seg0 + g.nseg, obj_acc, chg_acc);
    batch_block_partials(obj_acc, chg_acc, a.partials, blockIdx.x);
}

// objective of the last iterate (DESC_PGD.m:233), same workgroup table: thread t of workgroup g adds the cycles c0 + t, c0 + t + 256, ...
__global__ __launch_bounds__(256) void k_batch_objective(const double* w0, const double* w1, const double* S0v, const double* S1v, const int32_t* cum,
                                                         const int32_t* e_jk, const int32_t* e_ki, const BatchWg* wg, const BatchState* state,
                                                         int parity, double* partials) {
    const BatchWg g = wg[blockIdx.x];
    if (state[g.prob].stop) return;
    const double* w = parity ? w1 : w0;
    const double* S = parity ? S1v : S0v;
    const int c0 = cum[g.seg0], c1 = cum[g.seg0 + g.nseg];
    double acc = 0.0;
    for (int c = c0 + (int)threadIdx.x; c < c1; c += 256) acc += w[c] * (S[e_jk[c]] + S[e_ki[c]]);
    batch_block_partials(acc, 0.0, partials, blockIdx.x);
}

struct BatchFinArgs {
    const double* partials; BatchState* st; const BatchProb* prob; double* obj_trace; double* avg_trace; int32_t* running;
    double stop_tol; int32_t iters_cap, t, patience, last_only;
};
// One wave per problem: the problem's workgroup partials in fixed order, then the traces and the stop rule of DESC_PGD.m:232-257 for the
// iteration whose sums just became known.  last_only: the partials come from k_batch_objective after the final sweep t and hold obj(t);
// otherwise they come from sweep t: obj(t - 1) and sum |dS| of sweep t.
__global__ __launch_bounds__(64) void k_batch_finalize(BatchFinArgs f) {
    const int b = blockIdx.x;
    BatchState* st = f.st + b;
    if (st->stop) return;
    const BatchProb pb = f.prob[b];
    const int lane = threadIdx.x;
    double o = 0.0, ch = 0.0;
    for (int i = lane; i < pb.nwg; i += 64) {
        o += f.partials[2 * (int64_t)(pb.wg0 + i)];
        ch += f.partials[2 * (int64_t)(pb.wg0 + i) + 1];
    }
    o = group_sum<64>(o); ch = group_sum<64>(ch);
    if (lane != 0) return;
    double* obj = f.obj_trace + (int64_t)b * f.iters_cap;
    double* avg = f.avg_trace + (int64_t)b * f.iters_cap;
    const int t = f.t;
    const int it = f.last_only ? t : t - 1;          // iteration whose objective is o
    if (!f.last_only) avg[t - 1] = ch / (double)pb.m;                                   // :232
    if (it >= 1) {
        obj[it - 1] = o;                                                                // :233
        if (it > 1 && obj[it - 2] - obj[it - 1] < f.stop_tol) {                         // :243
            st->misses += 1;
            if (st->misses >= f.patience) {                                             // :245-246
                st->stop = 1; st->iters_run = it; st->final_parity = it & 1;
                atomicSub(f.running, 1);             // an integer count of the problems still running: the one word the host polls
            }
        } else {
            st->misses = 0;                                                             // :255
        }
    }
}

// wijk = 1/cnt, S_vec(IJ) = wijk_seg * S0_seg'  (DESC_PGD.m:151-157); one wave per edge (segments hold <= 64 cycles)
__global__ __launch_bounds__(256) void k_batch_init(const int32_t* cum, const int32_t* pos_edge, const double* S0, double* w, double* S_a, double* S_b,
                                                    int n_seg) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l = wid; l < n_seg; l += nw) {
        const int base = cum[l], cnt = cum[l + 1] - base;
        const double w0 = 1.0 / (double)cnt;
        double s = 0.0;
        for (int t = lane; t < cnt; t += 64) { w[(int64_t)base + t] = w0; s += w0 * S0[(int64_t)base + t]; }
        s = group_sum<64>(s);
        if (lane == 0) { S_a[pos_edge[l]] = s; S_b[pos_edge[l]] = s; }
    }
}

__global__ __launch_bounds__(256) void k_batch_fill(double* a, double* b, int64_t n, double v) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) { a[i] = v; b[i] = v; }
}

// Cycle inconsistency (DESC_PGD.m:129-147) of the whole batch: one wave per edge with cycles, lanes over its cycles.  ind_i, ind_j and kk
// hold the problems' LOCAL node ids (only compared with each other), e_jk / e_ki / pos_edge global edge ids into the concatenated rij.
__global__ __launch_bounds__(256) void k_batch_cycle_d(const int32_t* cum, const int32_t* pos_edge, const int32_t* ind_i, const int32_t* ind_j,
                                                       const int32_t* kk, const int32_t* e_jk, const int32_t* e_ki, const double* rij, double* S0,
                                                       int n_seg) {
    const int lane = threadIdx.x & 63;
    const int64_t wid = ((int64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    const int64_t nw = ((int64_t)gridDim.x * 256) >> 6;
    for (int64_t l = wid; l < n_seg; l += nw) {
        const int base = cum[l], cnt = cum[l + 1] - base;
        const int e = pos_edge[l], i = ind_i[e], j = ind_j[e];
        double A[9];
        for (int t = 0; t < 9; ++t) A[t] = rij[9 * (int64_t)e + t];
        for (int q = lane; q < cnt; q += 64) {
            const int64_t c = (int64_t)base + q;
            const int k = kk[c];
            const double tr = cycle_trace(A, rij + 9 * (int64_t)e_jk[c], !(j < k), rij + 9 * (int64_t)e_ki[c], !(k < i));
            S0[c] = abs_acos_ext((tr - 1.0) / 2.0) / M_PI;
        }
    }
}

// Before the download: problem b's final iterate sits in the buffers of parity (stopped ? final_parity : T & 1); where that is 1, copy
// its range of buffer 1 into buffer 0.  blockIdx.x = problem, off = its ranges (edges or cycles).
__global__ __launch_bounds__(256) void k_batch_settle(double* buf0, const double* buf1, const int64_t* off, const BatchState* state, int T) {
    const int b = blockIdx.x;
    const BatchState st = state[b];
    const int par = st.stop ? st.final_parity : (T & 1);
    if (!par) return;
    const int64_t lo = off[b], hi = off[b + 1];
    for (int64_t i = lo + (int64_t)blockIdx.y * 256 + threadIdx.x; i < hi; i += (int64_t)gridDim.y * 256) buf0[i] = buf1[i];
}

// desc_pgd_batch_create_on: the workgroup table formed on the device from one 16-byte record per problem, entry for entry the table
// batch_finish cuts on the host.  blockIdx.x = problem.
struct BatchWgSeed { int32_t seg0, m_pos, G, per; };
__global__ __launch_bounds__(256) void k_batch_wg_table(const BatchProb* prob, const BatchWgSeed* seed, BatchWg* wg) {
    const int b = blockIdx.x;
    const BatchProb pd = prob[b];
    const BatchWgSeed s = seed[b];
    for (int t = threadIdx.x; t < pd.nwg; t += 256) {
        const int l = t * s.per;
        wg[pd.wg0 + t] = BatchWg{b, s.seg0 + l, min(s.per, s.m_pos - l), s.G};
    }
}

}  // namespace
}  // namespace desc

using namespace desc;

struct desc_pgd_batch : desc::BatchDevice {     // device, stream, arena, events
    int32_t count = 0;
    std::vector<desc_structure*> st;          // per problem, local ids (desc_pgd_batch_get_structure)
    hvec<int64_t> edge_off, cycle_off, seg_off;
    hvec<int32_t> n_sample;
    int64_t M = 0, MC = 0, MP = 0;            // edges, cycles, segments of the whole batch
    int32_t nwg = 0;
    int32_t *d_cum = nullptr, *d_pos = nullptr, *d_ejk = nullptr, *d_eki = nullptr, *d_ikj = nullptr, *d_jki = nullptr;
    double *d_S0 = nullptr, *d_w[2] = {nullptr, nullptr}, *d_S[2] = {nullptr, nullptr};
    double *d_am[2] = {nullptr, nullptr}, *d_av[2] = {nullptr, nullptr};
    double *d_nv = nullptr, *d_partials = nullptr, *d_obj = nullptr, *d_avg = nullptr;
    int64_t trace_cap = 0;                    // doubles in d_obj / d_avg
    BatchState* d_state = nullptr;
    BatchWg* d_wg = nullptr;
    BatchProb* d_prob = nullptr;
    int64_t *d_edge_off = nullptr, *d_cycle_off = nullptr;
    int32_t* d_running = nullptr;
    double ms_cycle_d = 0;
    // a handle whose index arrays were made by the device builder (batch_structure.hip): st[b] is filled at the first
    // desc_pgd_batch_get_structure from the arrays below (blocks of the arena); the plain run never downloads them
    int32_t built_where = DESC_BUILD_HOST;
    hvec<desc::BatchPlan> plan;
    hvec<int64_t> prob_n;
    int32_t *d_kk = nullptr, *d_codeg = nullptr;
    bool st_ready = true;
    double ms_lap[desc::BATCH_BUILD_LAPS] = {0, 0, 0, 0, 0};
    std::shared_ptr<desc::PbSet> set;         // desc_pgd_batch_create_on: the owner of the edge list, the CSR and the rotations
    ~desc_pgd_batch() {
        close();                                  // the device first, as ever
        for (desc_structure* s : st) if (s) { structure_free_device(s); delete s; }
    }
};

namespace {

int batch_offsets(const desc_structure* const* s, int32_t count, int64_t* edge_off, int64_t* cycle_off, int64_t* seg_off) {
    edge_off[0] = cycle_off[0] = seg_off[0] = 0;
    for (int32_t b = 0; b < count; ++b) {
        if (!s[b]) return fail(DESC_ERR_INVALID, "problem %d: NULL structure", b);
        if (!s[b]->host_cycles) return fail(DESC_ERR_INVALID, "problem %d: the structure must be host-resident", b);
        edge_off[b + 1] = edge_off[b] + s[b]->m;
        cycle_off[b + 1] = cycle_off[b] + s[b]->m_cycle;
        seg_off[b + 1] = seg_off[b] + s[b]->m_pos;
    }
    if (cycle_off[count] >= (1ll << 31) - 1)
        return fail(DESC_ERR_TOO_LARGE, "the batch holds %lld cycles in total: the 2^31-1 index budget is exceeded, split the batch", (long long)cycle_off[count]);
    if (edge_off[count] >= (1ll << 30))
        return fail(DESC_ERR_TOO_LARGE, "the batch holds %lld edges in total: the 2^30 index budget is exceeded, split the batch", (long long)edge_off[count]);
    return DESC_OK;
}

// globalised copies of problem b's index arrays (T threads share the problems)
void batch_concat_fill(const desc_structure* const* s, int32_t count, const int64_t* edge_off, const int64_t* cycle_off, const int64_t* seg_off,
                       int32_t* pos_edge, int32_t* cum, int32_t* e_jk, int32_t* e_ki, int32_t* ikj, int32_t* jki) {
    for_each_problem(count, [&](int32_t b) {
        const desc_structure* q = s[b];
        const int32_t eo = (int32_t)edge_off[b], co = (int32_t)cycle_off[b];
        const int64_t so = seg_off[b], c0 = cycle_off[b];
        if (pos_edge) for (int64_t l = 0; l < q->m_pos; ++l) pos_edge[so + l] = q->pos_edge[l] + eo;
        if (cum) for (int64_t l = 0; l < q->m_pos; ++l) cum[so + l] = (int32_t)(q->cum_ind[l] + c0);
        for (int64_t c = 0; c < q->m_cycle; ++c) {
            if (e_jk) e_jk[c0 + c] = q->e_jk[c] + eo;
            if (e_ki) e_ki[c0 + c] = q->e_ki[c] + eo;
            if (ikj) ikj[c0 + c] = q->ikj[c] < 0 ? -1 : q->ikj[c] + co;
            if (jki) jki[c0 + c] = q->jki[c] < 0 ? -1 : q->jki[c] + co;
        }
    });
    if (cum) cum[seg_off[count]] = (int32_t)cycle_off[count];
}

// the plugin's step of iteration t (as make_step of pgd.hip: one GetStep call per iteration, the counter advances first)
StepArgs batch_step(const desc_pgd_batch* h, const desc_params& p, int t, int rd, int wr, bool* adam) {
    StepArgs s{};
    s.adam_m = h->d_am[rd]; s.adam_v = h->d_av[rd]; s.adam_m_out = h->d_am[wr]; s.adam_v_out = h->d_av[wr];
    *adam = plugin_step(p, p.t0 + t, s);
    return s;
}

int batch_finish(const desc_problem* probs, desc_pgd_batch* h, const int32_t* d_kk, const int32_t* d_ii, const int32_t* d_jj, const PbSet* set);

// set (nullable, here and below): the resident problem set a desc_pgd_batch_create_on builds on.  probs then views the set's host
// endpoints (no rotations), nothing is validated again, and the edge list and the rotations on the device are the set's.
int batch_create(const desc_problem* probs, int32_t count, const desc_params* p, const uint64_t* seeds, desc_pgd_batch* h, const PbSet* set = nullptr) {
    auto t0 = std::chrono::steady_clock::now();
    h->count = count; h->built_where = DESC_BUILD_HOST; h->st_ready = true;
    const int32_t nmin = p->n_sample_min > 0 ? p->n_sample_min : 30;
    for (int32_t b = 0; b < count && !set; ++b) {
        int rc = validate_problem(&probs[b], true);
        if (rc) { const std::string msg = desc_last_error(); return fail(rc, "problem %d: %s", b, msg.c_str()); }
    }
    // a-1..a-3 per problem on the host: local ids, so the structure is the one desc_structure_build gives for the problem alone
    h->st.assign((size_t)count, nullptr);
    hvec<int32_t> rcs((size_t)count, DESC_OK);
    std::vector<std::string> msgs((size_t)count);
    for_each_problem(count, [&](int32_t b) {
        struct Serial { bool was; Serial(bool on) : was(g_structure_serial) { g_structure_serial = on; } ~Serial() { g_structure_serial = was; } };
        Serial serial(count > 1);                // builders side by side: none of them starts threads of its own (16 host threads at most)
        desc_structure* s = new desc_structure();
        h->st[(size_t)b] = s;
        rcs[(size_t)b] = build_structure_host(&probs[b], nmin, seeds ? seeds[b] : p->seed, s);
        if (rcs[(size_t)b]) msgs[(size_t)b] = desc_last_error();            // the error text is per thread
    });
    for (int32_t b = 0; b < count; ++b)
        if (rcs[(size_t)b]) return fail(rcs[(size_t)b], "problem %d: %s", b, msgs[(size_t)b].c_str());
    h->n_sample.resize((size_t)count);
    for (int32_t b = 0; b < count; ++b) {
        const desc_structure* s = h->st[(size_t)b];
        h->n_sample[(size_t)b] = s->n_sample;
        if (s->n_sample > 64 || s->max_cnt > 64)
            return fail(DESC_ERR_INVALID, "problem %d: n_sample = %d exceeds 64 (segments longer than one wavefront): solve it with DESC_PGD", b, s->n_sample);
    }
    h->edge_off.assign((size_t)count + 1, 0); h->cycle_off.assign((size_t)count + 1, 0); h->seg_off.assign((size_t)count + 1, 0);
    int rc = batch_offsets(h->st.data(), count, h->edge_off.data(), h->cycle_off.data(), h->seg_off.data());
    if (rc) return rc;
    h->M = h->edge_off[(size_t)count]; h->MC = h->cycle_off[(size_t)count]; h->MP = h->seg_off[(size_t)count];
    if (count == 0) return DESC_OK;

    const size_t M = (size_t)h->M, MC = (size_t)h->MC, MP = (size_t)h->MP;
    hvec<int32_t> pos(MP), cum(MP + 1), ejk(MC), eki(MC), ikj(MC), jki(MC), kk(MC), ii(set ? 0 : M), jj(set ? 0 : M);
    batch_concat_fill(h->st.data(), count, h->edge_off.data(), h->cycle_off.data(), h->seg_off.data(), pos.data(), cum.data(), ejk.data(), eki.data(),
                      ikj.data(), jki.data());
    for (int32_t b = 0; b < count; ++b) {
        const desc_structure* s = h->st[(size_t)b];
        if (s->m_cycle) std::memcpy(kk.data() + h->cycle_off[(size_t)b], s->k.data(), sizeof(int32_t) * (size_t)s->m_cycle);
        if (s->m && !set) {
            std::memcpy(ii.data() + h->edge_off[(size_t)b], probs[b].ind_i, sizeof(int32_t) * (size_t)s->m);
            std::memcpy(jj.data() + h->edge_off[(size_t)b], probs[b].ind_j, sizeof(int32_t) * (size_t)s->m);
        }
    }
    h->plan.resize((size_t)count);                   // what the workgroup table is cut from
    for (int32_t b = 0; b < count; ++b) {
        const desc_structure* s = h->st[(size_t)b];
        BatchPlan& q = h->plan[(size_t)b];
        q = BatchPlan{};
        q.m_pos = s->m_pos; q.m_cycle = s->m_cycle; q.n_sample = s->n_sample; q.max_cnt = s->max_cnt;
    }
    if ((rc = h->open(set ? set->device : p->device, "DESC_PGD_batch"))) return rc;           // nothing above touched the device
    int32_t* d_kk = nullptr;
    const int32_t *d_ii = set ? set->d_ii : nullptr, *d_jj = set ? set->d_jj : nullptr;
    if ((rc = h->upload(&h->d_cum, cum.data(), MP + 1))) return rc;
    if ((rc = h->upload(&h->d_pos, pos.data(), MP))) return rc;
    if ((rc = h->upload(&h->d_ejk, ejk.data(), MC))) return rc;
    if ((rc = h->upload(&h->d_eki, eki.data(), MC))) return rc;
    if ((rc = h->upload(&h->d_ikj, ikj.data(), MC))) return rc;
    if ((rc = h->upload(&h->d_jki, jki.data(), MC))) return rc;
    if ((rc = h->upload(&d_kk, kk.data(), MC))) return rc;
    if (!set && ((rc = h->upload(&d_ii, ii.data(), M)) || (rc = h->upload(&d_jj, jj.data(), M)))) return rc;
    DESC_HIP(hipStreamSynchronize(h->stream));         // the index arrays are on the device: the staging vectors go out of scope below
    h->ms_structure = ms_since(t0);
    return batch_finish(probs, h, d_kk, d_ii, d_jj, set);
}

// Behind either builder, once the index arrays are on the device: the workgroup table, the small tables, the rotations, the state
// buffers, and S0_long of the whole batch in one launch.
int batch_finish(const desc_problem* probs, desc_pgd_batch* h, const int32_t* d_kk, const int32_t* d_ii, const int32_t* d_jj, const PbSet* set) {
    auto t1 = std::chrono::steady_clock::now();
    const int32_t count = h->count;
    const size_t M = (size_t)h->M, MC = (size_t)h->MC, MP = (size_t)h->MP;
    int rc;
    // the workgroup table: a problem's segments in runs of BATCH_PASSES x 4 waves x 64/G, counted from its own first segment
    hvec<BatchWg> wg;
    hvec<BatchProb> pr((size_t)count);
    hvec<BatchWgSeed> seed(set ? (size_t)count : 0);   // on a resident set the table is cut on the device: O(B) bytes go up, not O(segments)
    int64_t nwg = 0;
    for (int32_t b = 0; b < count; ++b) {
        const BatchPlan& s = h->plan[(size_t)b];
        const int G = s.max_cnt <= 16 ? 16 : s.max_cnt <= 32 ? 32 : 64;
        const int64_t per = (int64_t)BATCH_PASSES * 4 * (64 / G);
        pr[(size_t)b].wg0 = (int32_t)nwg; pr[(size_t)b].m = probs[b].m;
        if (!set)
            for (int64_t l = 0; l < s.m_pos; l += per)
                wg.push_back(BatchWg{b, (int32_t)(h->seg_off[(size_t)b] + l), (int32_t)std::min<int64_t>(per, s.m_pos - l), G});
        else
            seed[(size_t)b] = BatchWgSeed{(int32_t)h->seg_off[(size_t)b], (int32_t)s.m_pos, G, (int32_t)per};
        nwg += (s.m_pos + per - 1) / per;
        pr[(size_t)b].nwg = (int32_t)nwg - pr[(size_t)b].wg0;
    }
    h->nwg = (int32_t)nwg;
    const double* d_rij = set ? set->d_rij : nullptr;
    if ((rc = h->upload(&h->d_prob, pr.data(), pr.size()))) return rc;
    if (!set) {
        if ((rc = h->upload(&h->d_wg, wg.data(), wg.size()))) return rc;
    } else {
        BatchWgSeed* d_seed = nullptr;
        if ((rc = h->upload(&d_seed, seed.data(), seed.size())) || (rc = h->mem.alloc(&h->d_wg, (size_t)nwg))) return rc;
        hipLaunchKernelGGL(k_batch_wg_table, dim3((unsigned)count), dim3(256), 0, h->stream, h->d_prob, d_seed, h->d_wg);
        DESC_HIP(hipGetLastError());
    }
    if ((rc = h->upload(&h->d_edge_off, h->edge_off.data(), h->edge_off.size()))) return rc;
    if ((rc = h->upload(&h->d_cycle_off, h->cycle_off.data(), h->cycle_off.size()))) return rc;
    double nv[65];
    nv[0] = 0.0;
    for (int c = 1; c <= 64; ++c) nv[c] = 1.0 / std::pow((double)c, 0.5);             // ones/(nsample^0.5), DESC_PGD.m:199
    if ((rc = h->upload(&h->d_nv, nv, 65))) return rc;
    hvec<double> rij;
    if (!set) {
        rij = stage_rotations(probs, count, h->edge_off);
        if ((rc = h->upload(&d_rij, rij.data(), 9 * M))) return rc;
    }
    if ((rc = h->mem.alloc(&h->d_S0, MC))) return rc;
    for (int q = 0; q < 2; ++q) {
        if ((rc = h->mem.alloc(&h->d_w[q], MC))) return rc;
        if ((rc = h->mem.alloc(&h->d_S[q], M))) return rc;
    }
    if ((rc = h->mem.alloc(&h->d_partials, 2 * (size_t)std::max(h->nwg, 1)))) return rc;
    if ((rc = h->mem.alloc(&h->d_state, (size_t)count))) return rc;
    if ((rc = h->mem.alloc(&h->d_running, 1))) return rc;
    DESC_HIP(hipMemsetAsync(h->d_partials, 0, sizeof(double) * 2 * (size_t)std::max(h->nwg, 1), h->stream));
    DESC_HIP(hipStreamSynchronize(h->stream));         // the staging vectors go out of scope below
    h->ms_upload = ms_since(t1);
    // S0_long of the whole batch in one launch
    auto t2 = std::chrono::steady_clock::now();
    if (MP > 0) {
        hipLaunchKernelGGL(k_batch_cycle_d, dim3(grid_for((int64_t)MP, 4096, 4)), dim3(256), 0, h->stream, h->d_cum, h->d_pos, d_ii, d_jj, d_kk, h->d_ejk,
                           h->d_eki, d_rij, h->d_S0, (int)MP);
        DESC_HIP(hipGetLastError());
    }
    DESC_HIP(hipStreamSynchronize(h->stream));
    h->ms_cycle_d = ms_since(t2);
    return DESC_OK;
}

// The device builder (batch_structure.hip) in place of the per-problem host builds, the concatenation and the seven uploads.  May
// return BATCH_BUILD_FALLBACK: the caller then builds the same handle on the host.
int batch_create_device(const desc_problem* probs, int32_t count, const desc_params* p, const uint64_t* seeds, desc_pgd_batch* h,
                        const PbSet* set = nullptr) {
    auto t0 = std::chrono::steady_clock::now();
    h->count = count; h->built_where = DESC_BUILD_DEVICE;
    const int32_t nmin = p->n_sample_min > 0 ? p->n_sample_min : 30;
    BatchBuilt bb;
    int rc = batch_structure_device(h, probs, count, nmin, p->seed, seeds, set ? set->device : p->device, &bb, set);
    if (rc) return rc;
    h->st.assign((size_t)count, nullptr);
    h->st_ready = count == 0;
    h->prob_n.resize((size_t)count);
    h->n_sample.resize((size_t)count);
    for (int32_t b = 0; b < count; ++b) { h->prob_n[(size_t)b] = probs[b].n; h->n_sample[(size_t)b] = bb.plan[(size_t)b].n_sample; }
    h->plan = bb.plan; h->edge_off = bb.edge_off; h->cycle_off = bb.cycle_off; h->seg_off = bb.seg_off;
    h->M = h->edge_off[(size_t)count]; h->MC = h->cycle_off[(size_t)count]; h->MP = h->seg_off[(size_t)count];
    if (count == 0) return DESC_OK;
    h->d_cum = bb.d_cum; h->d_pos = bb.d_pos; h->d_ejk = bb.d_ejk; h->d_eki = bb.d_eki; h->d_ikj = bb.d_ikj; h->d_jki = bb.d_jki;
    h->d_kk = bb.d_kk; h->d_codeg = bb.d_codeg;
    for (int t = 0; t < BATCH_BUILD_LAPS; ++t) h->ms_lap[t] = bb.ms_lap[t];
    h->ms_structure = ms_since(t0);                    // batch_structure_device returned with the stream drained
    return batch_finish(probs, h, bb.d_kk, bb.d_ii, bb.d_jj, set);
}

// desc_pgd_batch_get_structure on a device-built handle, first request: the index arrays come down once, every problem's share less
// its offsets becomes a host-resident desc_structure.
int batch_structures_to_host(desc_pgd_batch* h) {
    if (h->st_ready) return DESC_OK;
    const size_t M = (size_t)h->M, MC = (size_t)h->MC, MP = (size_t)h->MP;
    hvec<int32_t> pos(MP), cum(MP + 1), ejk(MC), eki(MC), ikj(MC), jki(MC), kk(MC), cdg(M);
    DESC_HIP(hipSetDevice(h->device));
    DESC_HIP(hipStreamSynchronize(h->stream));
    const struct { int32_t* dst; const int32_t* src; size_t n; } copies[] = {
        {pos.data(), h->d_pos, MP}, {cum.data(), h->d_cum, MP + 1}, {ejk.data(), h->d_ejk, MC}, {eki.data(), h->d_eki, MC},
        {ikj.data(), h->d_ikj, MC}, {jki.data(), h->d_jki, MC}, {kk.data(), h->d_kk, MC}, {cdg.data(), h->d_codeg, M}};
    for (const auto& c : copies)
        if (c.n) DESC_HIP(hipMemcpy(c.dst, c.src, sizeof(int32_t) * c.n, hipMemcpyDeviceToHost));
    for (int32_t b = 0; b < h->count; ++b) {
        desc_structure* s = new desc_structure();
        h->st[(size_t)b] = s;
        const BatchPlan& q = h->plan[(size_t)b];
        const int64_t eo = h->edge_off[(size_t)b], co = h->cycle_off[(size_t)b], so = h->seg_off[(size_t)b];
        s->n = h->prob_n[(size_t)b]; s->m = h->edge_off[(size_t)b + 1] - eo; s->m_pos = q.m_pos; s->m_cycle = q.m_cycle;
        s->n_sample = q.n_sample; s->max_cnt = q.max_cnt; s->host_cycles = true;
        s->codeg.assign(cdg.begin() + eo, cdg.begin() + eo + s->m);
        s->pos_edge.resize((size_t)q.m_pos); s->cum_ind.resize((size_t)q.m_pos + 1);
        for (int64_t l = 0; l < q.m_pos; ++l) s->pos_edge[(size_t)l] = pos[(size_t)(so + l)] - (int32_t)eo;
        for (int64_t l = 0; l <= q.m_pos; ++l) s->cum_ind[(size_t)l] = (int64_t)cum[(size_t)(so + l)] - co;
        s->k.assign(kk.begin() + co, kk.begin() + co + q.m_cycle);
        s->e_jk.resize((size_t)q.m_cycle); s->e_ki.resize((size_t)q.m_cycle); s->ikj.resize((size_t)q.m_cycle); s->jki.resize((size_t)q.m_cycle);
        for (int64_t c = 0; c < q.m_cycle; ++c) {
            const size_t g = (size_t)(co + c);
            s->e_jk[(size_t)c] = ejk[g] - (int32_t)eo; s->e_ki[(size_t)c] = eki[g] - (int32_t)eo;
            s->ikj[(size_t)c] = ikj[g] < 0 ? -1 : ikj[g] - (int32_t)co; s->jki[(size_t)c] = jki[g] < 0 ? -1 : jki[g] - (int32_t)co;
        }
    }
    h->st_ready = true;
    return DESC_OK;
}

int batch_run(desc_pgd_batch* h, const desc_params* pin, desc_batch_result* r) {
    auto t0 = std::chrono::steady_clock::now();
    desc_params p = *pin;
    if (p.iters < 0) return fail(DESC_ERR_INVALID, "iters < 0");
    if (p.step_kind == DESC_STEP_EXTERNAL)
        return fail(DESC_ERR_INVALID, "step_kind DESC_STEP_EXTERNAL: a caller-supplied step rule does not run in batch mode, solve the problems one by one");
    if (p.step_kind < 0 || p.step_kind > 2) return fail(DESC_ERR_INVALID, "unknown step_kind %d", p.step_kind);
    if ((p.step_kind == DESC_STEP_PIECEWISE || (p.step_kind == DESC_STEP_HYBRID && p.hybrid_strategy == 1)) && !(p.decay_interval > 0))
        return fail(DESC_ERR_INVALID, "decay_interval must be > 0");
    if (p.patience <= 0) p.patience = 30;
    r->ms_structure = h->ms_structure; r->ms_upload = h->ms_upload; r->ms_cycle_d = h->ms_cycle_d; r->ms_pgd = 0.0;
    const int32_t count = h->count;
    if (count == 0) { r->ms_total = ms_since(t0); return DESC_OK; }
    if (!r->iters_run) return fail(DESC_ERR_INVALID, "result.iters_run is NULL");
    if (!r->s_vec && h->M > 0) return fail(DESC_ERR_INVALID, "result.s_vec is NULL");
    DESC_HIP(hipSetDevice(h->device));
    const bool adam = p.step_kind == DESC_STEP_HYBRID && p.hybrid_strategy == 0;
    const size_t M = (size_t)h->M, MC = (size_t)h->MC;
    const int cap = std::max(1, p.iters);
    int rc;
    if ((int64_t)cap * count > h->trace_cap) {         // blocks of earlier, shorter runs stay in the arena until destroy
        if ((rc = h->mem.alloc(&h->d_obj, (size_t)cap * count))) return rc;
        if ((rc = h->mem.alloc(&h->d_avg, (size_t)cap * count))) return rc;
        h->trace_cap = (int64_t)cap * count;
    }
    if (adam && !h->d_am[0])
        for (int q = 0; q < 2; ++q) {
            if ((rc = h->mem.alloc(&h->d_am[q], MC))) return rc;
            if ((rc = h->mem.alloc(&h->d_av[q], MC))) return rc;
        }
    // ---- init (DESC_PGD.m:148-167)
    DESC_HIP(hipMemsetAsync(h->d_state, 0, sizeof(BatchState) * (size_t)count, h->stream));
    DESC_HIP(hipMemsetAsync(h->d_obj, 0, sizeof(double) * (size_t)cap * count, h->stream));
    DESC_HIP(hipMemsetAsync(h->d_avg, 0, sizeof(double) * (size_t)cap * count, h->stream));
    DESC_HIP(hipMemcpyAsync(h->d_running, &count, sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    if (adam) {
        const bool carry = p.t0 > 0 && r->adam_m && r->adam_v && MC > 0;     // HybridGradient keeps m_t / v_t between calls
        for (int q = 0; q < 2; ++q) {
            DESC_HIP(hipMemsetAsync(h->d_am[q], 0, sizeof(double) * std::max<size_t>(MC, 1), h->stream));
            DESC_HIP(hipMemsetAsync(h->d_av[q], 0, sizeof(double) * std::max<size_t>(MC, 1), h->stream));
        }
        if (carry) {                                   // into the parity sweep 1 reads
            DESC_HIP(hipMemcpyAsync(h->d_am[0], r->adam_m, sizeof(double) * MC, hipMemcpyHostToDevice, h->stream));
            DESC_HIP(hipMemcpyAsync(h->d_av[0], r->adam_v, sizeof(double) * MC, hipMemcpyHostToDevice, h->stream));
        }
    }
    if (M > 0) hipLaunchKernelGGL(k_batch_fill, dim3(grid_for((int64_t)M, 1024)), dim3(256), 0, h->stream, h->d_S[0], h->d_S[1], (int64_t)M, 1.0);   // :148
    if (h->MP > 0)
        hipLaunchKernelGGL(k_batch_init, dim3(grid_for(h->MP, 4096, 4)), dim3(256), 0, h->stream, h->d_cum, h->d_pos, h->d_S0, h->d_w[0], h->d_S[0], h->d_S[1],
                           (int)h->MP);
    DESC_HIP(hipGetLastError());

    // ---- loop (:182-261): per iteration one sweep of the whole batch + one bookkeeping wave per problem
    if ((rc = h->timer_begin())) return rc;
    const int chunk = p.check_every > 0 ? p.check_every : 32;
    BatchFinArgs f{h->d_partials, h->d_state, h->d_prob, h->d_obj, h->d_avg, h->d_running, p.stop_tol, cap, 0, p.patience, 0};
    int T = 0;
    while (T < p.iters) {
        const int upto = std::min(p.iters, T + chunk);
        for (int t = T + 1; t <= upto; ++t) {
            const int rd = (t - 1) & 1, wr = t & 1;
            if (h->nwg > 0) {
                BatchArgs a{};
                a.cum = h->d_cum; a.pos_edge = h->d_pos; a.e_jk = h->d_ejk; a.e_ki = h->d_eki; a.ikj = h->d_ikj; a.jki = h->d_jki; a.S0 = h->d_S0;
                a.w_old = h->d_w[rd]; a.w_new = h->d_w[wr]; a.S_old = h->d_S[rd]; a.S_new = h->d_S[wr]; a.nv_tab = h->d_nv; a.partials = h->d_partials;
                a.state = h->d_state; a.wg = h->d_wg;
                bool is_adam = false;
                a.st = batch_step(h, p, t, rd, wr, &is_adam);
                if (is_adam) hipLaunchKernelGGL((k_batch_sweep<DESC_STEP_HYBRID>), dim3(h->nwg), dim3(256), 0, h->stream, a);
                else hipLaunchKernelGGL((k_batch_sweep<DESC_STEP_CONSTANT>), dim3(h->nwg), dim3(256), 0, h->stream, a);
            }
            f.t = t; f.last_only = 0;
            hipLaunchKernelGGL(k_batch_finalize, dim3(count), dim3(64), 0, h->stream, f);
        }
        T = upto;
        DESC_HIP(hipGetLastError());
        if (T < p.iters) {                             // the one word the host polls
            int32_t running = 0;
            DESC_HIP(hipMemcpyAsync(&running, h->d_running, sizeof running, hipMemcpyDeviceToHost, h->stream));
            DESC_HIP(hipStreamSynchronize(h->stream));
            if (running == 0) break;
        }
    }
    // objective of the last sweep (:233) and its stop test, for the problems still running
    if (T >= 1) {
        if (h->nwg > 0)
            hipLaunchKernelGGL(k_batch_objective, dim3(h->nwg), dim3(256), 0, h->stream, h->d_w[0], h->d_w[1], h->d_S[0], h->d_S[1], h->d_cum, h->d_ejk, h->d_eki,
                               h->d_wg, h->d_state, T & 1, h->d_partials);
        f.t = T; f.last_only = 1;
        hipLaunchKernelGGL(k_batch_finalize, dim3(count), dim3(64), 0, h->stream, f);
    }
    if ((rc = h->timer_end())) return rc;
    // ---- every problem's final iterate into buffer 0
    const dim3 gE(count, std::max(1, std::min<int>(64, (int)((M / (size_t)count + 255) / 256))));
    const dim3 gC(count, std::max(1, std::min<int>(64, (int)((MC / (size_t)count + 255) / 256))));
    hipLaunchKernelGGL(k_batch_settle, gE, dim3(256), 0, h->stream, h->d_S[0], h->d_S[1], h->d_edge_off, h->d_state, T);
    if (r->w) hipLaunchKernelGGL(k_batch_settle, gC, dim3(256), 0, h->stream, h->d_w[0], h->d_w[1], h->d_cycle_off, h->d_state, T);
    const bool adam_out = adam && r->adam_m && r->adam_v;
    if (adam_out) {
        hipLaunchKernelGGL(k_batch_settle, gC, dim3(256), 0, h->stream, h->d_am[0], h->d_am[1], h->d_cycle_off, h->d_state, T);
        hipLaunchKernelGGL(k_batch_settle, gC, dim3(256), 0, h->stream, h->d_av[0], h->d_av[1], h->d_cycle_off, h->d_state, T);
    }
    DESC_HIP(hipGetLastError());
    DESC_HIP(hipStreamSynchronize(h->stream));
    float ms = 0;
    if ((rc = h->timer_ms(&ms))) return rc;
    r->ms_pgd = ms;
    // ---- download
    hvec<BatchState> st((size_t)count);
    DESC_HIP(hipMemcpy(st.data(), h->d_state, sizeof(BatchState) * (size_t)count, hipMemcpyDeviceToHost));
    if (M) DESC_HIP(hipMemcpy(r->s_vec, h->d_S[0], sizeof(double) * M, hipMemcpyDeviceToHost));
    if (r->w && MC) DESC_HIP(hipMemcpy(r->w, h->d_w[0], sizeof(double) * MC, hipMemcpyDeviceToHost));
    if (adam_out && MC) {                              // the state after exactly iters_run[b] GetStep calls of problem b
        DESC_HIP(hipMemcpy(r->adam_m, h->d_am[0], sizeof(double) * MC, hipMemcpyDeviceToHost));
        DESC_HIP(hipMemcpy(r->adam_v, h->d_av[0], sizeof(double) * MC, hipMemcpyDeviceToHost));
    }
    hvec<double> tr;
    for (int which = 0; which < 2; ++which) {
        double* dst = which ? r->avg_change_trace : r->obj_trace;
        if (!dst || p.iters == 0) continue;
        tr.resize((size_t)cap * count);
        DESC_HIP(hipMemcpy(tr.data(), which ? h->d_avg : h->d_obj, sizeof(double) * tr.size(), hipMemcpyDeviceToHost));
        for (int32_t b = 0; b < count; ++b) {
            const int it = st[(size_t)b].stop ? st[(size_t)b].iters_run : T;
            double* row = dst + (size_t)b * (size_t)p.iters;
            std::memcpy(row, tr.data() + (size_t)b * cap, sizeof(double) * (size_t)it);
            std::memset(row + it, 0, sizeof(double) * (size_t)(p.iters - it));     // sweep t + 1 of a problem stopped at t left an entry behind
        }
    }
    for (int32_t b = 0; b < count; ++b) {
        const int it = st[(size_t)b].stop ? st[(size_t)b].iters_run : T;
        r->iters_run[b] = it;
        if (r->t_end) r->t_end[b] = p.t0 + it;
    }
    r->ms_total = ms_since(t0);
    return DESC_OK;
}

}  // namespace

extern "C" {

int desc_pgd_batch_create(const desc_problem* probs, int32_t count, const desc_params* p, const uint64_t* seeds, desc_pgd_batch** out) {
    return batch_create_guarded("desc_pgd_batch_create", out, probs, count,
                                [&](desc_pgd_batch* h) { return batch_create(probs, count, p, seeds, h); }, p != nullptr);
}

int desc_pgd_batch_create_where(const desc_problem* probs, int32_t count, const desc_params* p, const uint64_t* seeds, int32_t where,
                                desc_pgd_batch** out) {
    if (where != DESC_BUILD_HOST && where != DESC_BUILD_DEVICE) {
        if (out) *out = nullptr;
        return fail(DESC_ERR_INVALID, "where = %d: need DESC_BUILD_HOST or DESC_BUILD_DEVICE", (int)where);
    }
    return batch_create_guarded("desc_pgd_batch_create_where", out, probs, count, [&](desc_pgd_batch* h) {
        if (where == DESC_BUILD_DEVICE) {
            const int rc = batch_create_device(probs, count, p, seeds, h);
            if (rc != BATCH_BUILD_FALLBACK) return rc;
            h->close();                                // outside what the device builder stages: the same handle, built on the host
        }
        return batch_create(probs, count, p, seeds, h);
    }, p != nullptr);
}

int desc_pgd_batch_create_on(desc_problem_batch* set, const desc_params* p, const uint64_t* seeds, int32_t where, desc_pgd_batch** out) {
    if (where != DESC_BUILD_HOST && where != DESC_BUILD_DEVICE) {
        if (out) *out = nullptr;
        return fail(DESC_ERR_INVALID, "where = %d: need DESC_BUILD_HOST or DESC_BUILD_DEVICE", (int)where);
    }
    return batch_create_guarded("desc_pgd_batch_create_on", out, set, 0, [&](desc_pgd_batch* h) {
        const PbSet* s = set->s.get();
        const int32_t count = s->count;
        hvec<desc_problem> probs((size_t)count);        // views of the set's host endpoints: what either builder reads of a problem
        for (int32_t b = 0; b < count; ++b) {
            const int64_t eo = s->edge_off[(size_t)b];
            desc_problem& q = probs[(size_t)b];
            q.n = s->node_off[(size_t)b + 1] - s->node_off[(size_t)b]; q.m = s->edge_off[(size_t)b + 1] - eo;
            q.ind_i = s->ii.data() + eo; q.ind_j = s->jj.data() + eo; q.rij = nullptr;
        }
        h->set = set->s;                               // before the first device block of the handle: the set outlives what borrows from it
        if (where == DESC_BUILD_DEVICE) {
            const int rc = batch_create_device(probs.data(), count, p, seeds, h, s);
            if (rc != BATCH_BUILD_FALLBACK) return rc;
            h->close();                                // outside what the device builder stages: the same handle, built on the host
        }
        return batch_create(probs.data(), count, p, seeds, h, s);
    }, set != nullptr && p != nullptr);
}

int desc_pgd_batch_bytes(const desc_pgd_batch* h, int64_t* h2d, int64_t* d2h) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    if (h2d) *h2d = h->bytes_h2d;
    if (d2h) *d2h = h->bytes_d2h;
    return DESC_OK;
}

int32_t desc_pgd_batch_built_where(const desc_pgd_batch* h) { return h ? h->built_where : (int32_t)fail(DESC_ERR_INVALID, "NULL handle"); }

int desc_pgd_batch_build_laps(const desc_pgd_batch* h, double* ms) {
    if (!h || !ms) return fail(DESC_ERR_INVALID, "NULL argument");
    for (int t = 0; t < BATCH_BUILD_LAPS; ++t) ms[t] = h->ms_lap[t];
    return DESC_OK;
}

int desc_pgd_batch_sizes(const desc_pgd_batch* h, int32_t* count, int64_t* edge_off, int64_t* cycle_off, int32_t* n_sample) {
    if (!h) return fail(DESC_ERR_INVALID, "NULL handle");
    if (count) *count = h->count;
    if (edge_off) std::copy(h->edge_off.begin(), h->edge_off.end(), edge_off);
    if (cycle_off) std::copy(h->cycle_off.begin(), h->cycle_off.end(), cycle_off);
    if (n_sample) std::copy(h->n_sample.begin(), h->n_sample.end(), n_sample);
    return DESC_OK;
}

int desc_pgd_batch_get_structure(const desc_pgd_batch* h, int32_t b, desc_structure_view* view) {
    if (!h || !view) return fail(DESC_ERR_INVALID, "NULL argument");
    if (b < 0 || b >= h->count) return fail(DESC_ERR_INVALID, "problem %d out of range (the batch holds %d)", b, h->count);
    const int rc = no_throw("desc_pgd_batch_get_structure", [&]() -> int { return batch_structures_to_host(const_cast<desc_pgd_batch*>(h)); });
    if (rc) return rc;
    return desc_structure_get(h->st[(size_t)b], view);
}

int desc_pgd_batch_get_s0(desc_pgd_batch* h, double* s0) {
    if (!h || (!s0 && h->MC > 0)) return fail(DESC_ERR_INVALID, "NULL argument");
    if (h->MC == 0) return DESC_OK;
    DESC_HIP(hipSetDevice(h->device));
    DESC_HIP(hipStreamSynchronize(h->stream));
    DESC_HIP(hipMemcpy(s0, h->d_S0, sizeof(double) * (size_t)h->MC, hipMemcpyDeviceToHost));
    return DESC_OK;
}

int desc_pgd_batch_run(desc_pgd_batch* h, const desc_params* p, desc_batch_result* r) {
    return no_throw("desc_pgd_batch_run", [&]() -> int {
        if (!h || !p || !r) return fail(DESC_ERR_INVALID, "NULL argument");
        return batch_run(h, p, r);
    });
}

void desc_pgd_batch_destroy(desc_pgd_batch* h) { delete h; }

int desc_pgd_batch_concat(const desc_structure* const* s, int32_t count, int64_t* edge_off, int64_t* cycle_off, int64_t* seg_off,
                          int32_t* pos_edge, int32_t* cum, int32_t* e_jk, int32_t* e_ki, int32_t* ikj, int32_t* jki) {
    return no_throw("desc_pgd_batch_concat", [&]() -> int {
        if (count < 0 || (count > 0 && !s) || !edge_off || !cycle_off || !seg_off) return fail(DESC_ERR_INVALID, "NULL argument or negative count");
        int rc = batch_offsets(s, count, edge_off, cycle_off, seg_off);
        if (rc) return rc;
        batch_concat_fill(s, count, edge_off, cycle_off, seg_off, pos_edge, cum, e_jk, e_ki, ikj, jki);
        return DESC_OK;
    });
}

}  // extern "C"

// The PGD solver handle (struct desc_pgd), its allocation helpers, the sweep-instance types and the host functions that cross the units of
// the solver: the sweep units (sweep_gather.hip, sweep_node.hip, sweep_band.hip), pgd.hip, pgd_layout.hip, pgd_shard.hip and pgd_ext.hip.
#pragma once

#include <cstdlib>
#include <string>

#include "node_plan.h"
#include "pgd_device.h"

// ------------------------------------------------------------------- handle --
enum { VARIANT_GATHER = 1, VARIANT_NODE = 2 };

struct desc_pgd {
    int device = 0;
    hipStream_t stream = nullptr;
    int64_t n = 0, m = 0, m_pos = 0, m_cycle = 0;
    int32_t max_cnt = 0, n_sample = 0, max_deg = 0;
    int variant = VARIANT_GATHER;
    bool band_jmajor = false;   // band sweep: j-block-major units (large graphs) instead of contiguous ranges
    int grid = 0;               // sweep grid (multiple of 8)
    int obj_grid = 0;
    int colsum_grid = 0, colsum_stride = 0, colsum_cl = 16;     // colsum_cl: lanes per segment in k_colsum_node (8 when the runs are short)
    int colsum_fx_bits = 47;                                     // fixed-point position of the column sums: 62 - ceil(log2(max degree + 1))
    int colsum_nodes = 0;                                        // nodes k_colsum_node visits (sharded: those with segments of this rank in their row)
    int colsum_long = 0;                                         // nodes that get a whole workgroup in k_colsum_node (the rest: a wave each, sharded runs)
    int64_t colsum_entries = 0;                                  // (cycle, endpoint) pairs the column sums read: cycles whose mirror was sampled, per endpoint
    int64_t n_pieces = 0, n_bands = 0, piece_row_entries = 0;    // band sweep plan: pieces, bands, CSR entries of band rows loaded per sweep
    int band = 0;
    bool band_ok = false;       // k_sweep_band applies (segments <= 64 cycles, rows fit the LDS)
    bool small_ok = false;      // k_sweep_small: one rank, < 2 M cycles, segments of at most 64 cycles (the reference's demo sizes)
    int small_grid = 0;
    int band_grid = 0, band_rows = 0;
    size_t band_lds = 0;
    desc::PieceDesc* d_pieces = nullptr;
    int32_t* d_piece_ptr = nullptr;
    unsigned long long* d_wg_clock = nullptr;   // diagnostics: DESC_DEBUG_WGCLOCK
    int band_tail_first = 0, band_ntail = 0;    // shared tail of the band sweep (BandSweepArgs)
    int32_t* d_ticket = nullptr;
    int32_t* d_node_order = nullptr;            // column sums: the nodes gone through (one workgroup each, dispatched in index order); sharded: only those with owned segments
    int2* d_node_run = nullptr;                 // sharded runs: per node the run [x, y) of its row's CSR slots whose segments this rank owns (NULL: whole rows)
    hvec<void*> allocs;
    int uc_default = 0;         // which streamed arrays go to uncached memory (dalloc_stream)
    // common
    int32_t* d_cum = nullptr;
    double *d_S0 = nullptr, *d_w[2] = {nullptr, nullptr}, *d_S[2] = {nullptr, nullptr};
    double *d_adam_m[2] = {nullptr, nullptr}, *d_adam_v[2] = {nullptr, nullptr}, *d_nv = nullptr, *d_partials = nullptr;
    double *d_obj = nullptr, *d_avg = nullptr, *d_scratch = nullptr;
    desc::DevState* d_state = nullptr;
    // gather variant
    int32_t *d_pos_edge = nullptr, *d_ejk = nullptr, *d_eki = nullptr, *d_ikj = nullptr, *d_jki = nullptr;
    // node variant
    desc::EdgeInfo* d_einfo = nullptr;
    uint32_t* d_pk = nullptr;
    uint32_t* d_moff = nullptr;  // per CSR slot: start of its run in d_midx
    uint16_t* d_midx = nullptr;  // column index of every contributing cycle, in the order the column-sum pass reads them
    int2* d_adj_seg = nullptr;   // per CSR slot: slot_record() = {first contributing cycle of the incident segment, their number | (row node is the smaller endpoint) << 31}
    int32_t *d_rowptr = nullptr, *d_src_start = nullptr, *d_eslot = nullptr;
    desc::ChunkDesc* d_chunk_desc = nullptr;
    int nchunks = 0;
    double *d_T = nullptr, *d_Svec = nullptr;
    uint8_t* d_seg_perm = nullptr;     // natural in-segment offset of every device-order cycle
    // sharding (world == 1: the whole problem)
    int rank = 0, world = 1;
    int64_t seg_lo = 0, seg_hi = 0;     // device-order range of segments owned by this rank
    int64_t cyc_lo = 0, cyc_hi = 0;     // their cycles
    int ch_lo = 0;                      // first chunk owned
    int64_t slice_len = 0;              // doubles per rank in the S exchange buffer
    int64_t slice_S = 0;                // ... of which S values (the rest: SHARD_PARTS pairs of partials)
    desc_collectives coll{};            // fused protocol: the caller's collectives (RCCL entry points + communicator)
    hipStream_t comm_stream = nullptr;  // second stream: exchange + unpack overlap the next column-sum pass
    hipEvent_t ev_col = nullptr, ev_rs = nullptr, ev_sw = nullptr, ev_ag = nullptr;
    desc::StepArgs cur_step{}; bool cur_adam = false;      // sharded sweeps: the step of the sweep in progress (its exchange parts are separate launches)
    int unpack_pending = 0;             // fused protocol: sweep whose all-gathered S still has to be unpacked (on the compute stream, behind ev_ag)
    bool own_xbuf = false, force_coll = false;
    hvec<int64_t> rank_seg;      // world+1 segment boundaries
    double* x_T = nullptr;              // caller-bound exchange buffers (device): owner-sorted partial mirror sums (send)
    double* x_Trecv = nullptr;          // reduce-scattered mirror sums of the owned segments
    int32_t* d_xpos = nullptr;          // 2m: CSR slot -> position of its column sum in x_T (k_xpos)
    int32_t* d_spos = nullptr;          // 2m: CSR slot -> position of its edge's S in the gathered slices x_sall
    int2* d_xt = nullptr;               // m_pos (device order; owned segments filled): {ta, tb} = places of T1 / T2 in x_Trecv, ta also in the slice
    int64_t t_part = 0;                 // words per block of the exchange layout (one block per virtual owner = (rank, part))
    int xparts = 1;                     // exchange parts per rank (NodePlan::xparts): one reduce-scatter and one sweep launch each
    hvec<int64_t> xseg;                 // xparts + 1: device-order segment boundaries of this rank's parts
    hvec<int64_t> xslice_off;           // xparts: first edge of the part - first edge of the rank (offset of the part's S in the rank's slice)
    hvec<int> xpiece_base, xpiece_ptr_base, xtail_first, xntail;      // per part: where its pieces / piece_ptr start in d_pieces / d_piece_ptr, its shared tail
    hipEvent_t ev_rsx[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // fused protocol: reduce-scatter of part c done
    double* x_sall = nullptr;           //   world * slice_len
    bool borrowed_stream = false, objective_done = false;
    int last_parts = 0;                 // workgroup partials the last sharded sweep wrote
    int final_obj_T = -1;               // sweep count for which download already evaluated the objective
    int pending_fin = 0, pending_parts = 0;   // sweep whose bookkeeping (k_finalize) rides on the next column-sum launch
    int32_t* d_rank_seg = nullptr;
    int trace_cap = 0;          // allocated length of d_obj / d_avg (the largest budget this handle has seen)
    int iters_cap = 0;          // max(1, params.iters) of the last reset: what the caller's trace buffers hold
    // run state
    desc_params p{};
    bool armed = false;
    int t_done = 0;             // sweeps enqueued since reset
    int t_plugin = 0;           // plugin counter (PiecewiseStepSize.t / HybridGradient.t)
    double ms_upload = 0, ms_cycle_d = 0, ms_pgd = 0;
    std::string kname;
    std::string last_sweep;     // the sweep instance launched last, with its template arguments (desc_debug_last_sweep: tests assert which kernel ran)
    // caller-supplied step rule (desc_pgd_ext_*): the iteration cut at DESC_PGD.m:207
    int ext_phase = 0;          // 0 not begun | EXT_GRAD_DUE | EXT_STEP_DUE | EXT_STOPPED
    double* d_ext_io = nullptr; // m_cycle doubles in the reference's cycle order: host-mode staging of grad_long and of the step
    double* d_ext_out = nullptr;        // {average_change, objective, stop flag} of the iteration just applied
    hipEvent_t ev_ext[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};      // gradient pass [0,1]; apply pass [2,3]; objective + stop rule [3,4]
    double ext_ms[3] = {0, 0, 0};       // device time of the last gradient pass, apply pass, objective (desc_pgd_ext_laps)
};

namespace desc {

template <class T>
int dalloc(desc_pgd* h, T** p, size_t count) {
    *p = nullptr;
    void* q = nullptr;
    DESC_HIP(dev_alloc(&q, sizeof(T) * (count > 0 ? count : 1)));
    h->allocs.push_back(q);
    *p = (T*)q;
    return DESC_OK;
}
// The arrays the band sweep streams through exactly once per launch and never writes -- S0 (8 B per cycle) and the packed words (4 B) --
// live in UNCACHED device memory (MTYPE UC; devmem.hip): their lines do not stay in the L2, where the rows of S the sweep gathers from then
// keep their place.  Measured (profiles/r03_uncached_streams.txt, rocprofv3 sweep averages in one call): C4 1170 -> 1130 us (-3.4 %); the
// weights too (read, written, read again by the column sums): +17 %, not done; C5 / C2 / C3: see the file.  DESC_DEBUG_UNCACHED overrides
// the mask (1 weights, 2 S0, 4 packed words, 8 the column-index stream of the column sums, 16 their slot records; default 6 on graphs
// whose S does not fit the L2s, else 0).
template <class T>
int dalloc_stream(desc_pgd* h, T** p, size_t count, int bit) {
    const char* ev = std::getenv("DESC_DEBUG_UNCACHED");
    const int mask = ev ? std::atoi(ev) : h->uc_default;
    if (!(mask & bit)) return dalloc(h, p, count);
    *p = nullptr;
    void* q = nullptr;
    DESC_HIP(dev_alloc_uncached(&q, sizeof(T) * (count > 0 ? count : 1)));
    h->allocs.push_back(q);
    *p = (T*)q;
    return DESC_OK;
}
inline void dfree(desc_pgd* h, void* q) {
    if (!q) return;
    for (auto& x : h->allocs) if (x == q) { x = nullptr; break; }
    dev_free(q);
}

inline int set_device(const desc_pgd* h) { DESC_HIP(hipSetDevice(h->device)); return DESC_OK; }
inline int64_t local_cycles(const desc_pgd* h) { return h->variant == VARIANT_NODE ? h->cyc_hi - h->cyc_lo : h->m_cycle; }

template <class T>
int upload(desc_pgd* h, T* dst, const T* src, size_t count) {
    if (count) DESC_HIP(hipMemcpyAsync(dst, src, sizeof(T) * count, hipMemcpyHostToDevice, h->stream));
    return DESC_OK;
}

// ------------------------------------------------------------ sweep instances --
// Every instance of a sweep kernel that can be launched is written once, as an entry of its family's table.  The launch, the kernel's address
// (hipFuncSetAttribute, the occupancy query) and the names desc_debug_last_sweep and desc_pgd_kernel_name return all come from that entry; the
// rule from the longest segment to an entry's shape is one function per family.
struct SweepShape { int lps, E; };      // lanes per segment x cycles per lane (gather layout and k_sweep_small: E = 0)
template <class... A>
struct SweepInst {
    SweepShape sh;
    int NT;                             // threads per workgroup
    void (*kern[2])(A...);              // {constant step, Adam}; band sweep: {one rank, XT}
};
constexpr int STEP_OF[2] = {DESC_STEP_CONSTANT, DESC_STEP_HYBRID};      // the STEP argument of kern[adam]
template <class I, size_t N>
const I* sweep_inst(const I (&table)[N], SweepShape sh) {
    for (const I& i : table) if (i.sh.lps == sh.lps && i.sh.E == sh.E) return &i;
    fail(DESC_ERR_STATE, "no sweep instance of %d lanes per segment x %d cycles per lane", sh.lps, sh.E);
    return nullptr;
}
template <class... V>
std::string inst_name(const char* fmt, V... v) { char nm[64]; snprintf(nm, sizeof nm, fmt, v...); return nm; }

// ------------------------------------------------------------ the sweep units --
struct BandSweepArgs;
// sweep_gather.hip
int launch_gather(desc_pgd* h, const SweepArgs& a, bool adam);
int setup_gather(desc_pgd* h, const desc_problem* prob, const desc_structure* s, const double* shared_rij);
// sweep_node.hip
const SweepInst<NodeSweepArgs>* node_inst_of(SweepShape sh);
SweepShape node_shape(int c);
std::string node_prefix(SweepShape sh);
SweepShape small_shape(int c);
std::string small_prefix(SweepShape sh);
int launch_sweep_node_layout(desc_pgd* h, const NodeSweepArgs& a, bool adam, int part = 0);
int sweep_parts(const desc_pgd* h, bool adam, bool plain_path = false);
// sweep_band.hip
bool band_adam_ok(const desc_pgd* h);
SweepShape band_shape(const desc_pgd* h, bool adam);
const SweepInst<BandSweepArgs>* band_inst_of(const desc_pgd* h, bool adam);
std::string band_prefix(SweepShape sh);
int launch_band(desc_pgd* h, const NodeSweepArgs& a, bool adam, int part);      // for launch_sweep_node_layout (sweep_node.hip)

// -------------------------------------------------------- the other PGD units --
// pgd.hip
StepArgs make_step(desc_pgd* h, bool* adam, int rd, int wr);
size_t parts_cap(const desc_pgd* h);
double* obj_partials(const desc_pgd* h);
FinArgs fin_args(const desc_pgd* h, const double* partials, int nparts, int t, int last_only);
NodeSweepArgs node_sweep_args(const desc_pgd* h, int rd, int wr);
void launch_objective(desc_pgd* h, hipStream_t st, int par, int grid, double* partials);
void launch_unpack(desc_pgd* h, hipStream_t st, int g, double* S_a, double* S_b, const FinArgs& f);
constexpr int COLSUM_SHORT = 128;         // sharded runs: rows whose owned run has at most this many segments are summed by ONE wave (four nodes per workgroup)
int prepare_colsum(desc_pgd* h);
void launch_colsum(desc_pgd* h, hipStream_t st, const double* w, double* T, const int32_t* xpos, const FinArgs& fin);
// pgd_layout.hip
int setup_node(desc_pgd* h, const desc_problem* prob, const desc_structure* s, const double* shared_rij);
// pgd_shard.hip
int shard_unpack_pending(desc_pgd* h);

}  // namespace desc

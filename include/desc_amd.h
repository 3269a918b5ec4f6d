/* desc_amd.h -- C ABI of libdesc_amd.so (MI355X / gfx950 HIP implementation of the
 * DESC projected-gradient hot path).
 *
 * The reference (ColeWyeth/DESC) is pure MATLAB and has no FFI of its own; the
 * boundary this library replaces is the MATLAB function signature
 *     S_vec = DESC_PGD(Ind, RijMat, params)            Algorithms/DESC_PGD.m:14
 * (the same body is inlined in Algorithms/DESC.m:16-261, called from
 * Demo/compare_algorithms.m:72).  A MEX shim (matlab/desc_pgd_mex.c) or any other
 * FFI (ctypes: desc_amd/_lib.py) binds exactly the entry points below.  Plain
 * pointers and sizes only; no exceptions cross the boundary; every function
 * returns DESC_OK (0) or a negative error code, with text from desc_last_error().
 *
 * Conventions
 *   - all indices are 0-based int32 (the MATLAB side subtracts 1);
 *   - edges are rows (ind_i[l], ind_j[l]) with ind_i < ind_j, strictly sorted by
 *     (ind_i, ind_j) -- the order DESC_PGD.m:5,31-34 silently relies on;
 *   - rij is m x 9 doubles, block l = RijMat(:,:,l) in MATLAB column-major order
 *     (element (r,c) at rij[9*l + r + 3*c]), i.e. mxGetDoubles(RijMat) unchanged;
 *   - all arithmetic is IEEE double (the reference has no single precision).
 *   - the caller owns every host buffer it passes; the library owns device memory.
 *   - threads: any entry point may be called from any host thread, and DISTINCT objects (structures, device problems,
 *     solver handles, one-shot solves) may be in use on distinct threads at the same time -- a MATLAB worker pool or a
 *     serving process; the block / stream pools are locked, desc_last_error() is per thread.  One object must not be
 *     used from two threads at once.  (tests/test_gpu_parity.py::test_concurrent_solves_from_several_host_threads)
 */
#ifndef DESC_AMD_H
#define DESC_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DESC_OK              0
#define DESC_ERR_INVALID    -1   /* bad argument / unsorted Ind / out-of-range index     */
#define DESC_ERR_HIP        -2   /* HIP runtime error (no device, OOM, launch failure)   */
#define DESC_ERR_TOO_LARGE  -3   /* m_cycle or m exceeds the 2^31-1 / 2^30 index budget  */
#define DESC_ERR_STATE      -4   /* call order violated (e.g. iterate before reset)      */

/* step-size plugin kinds: params.Gradient of the reference (DESC_PGD.m:207) */
#define DESC_STEP_CONSTANT   0   /* Utils/ConstantStepSize.m:9-11   step = -lr*g                       */
#define DESC_STEP_PIECEWISE  1   /* Utils/PiecewiseStepSize.m:13-18 step = -lr/(fix(t/decay)+1)*g      */
#define DESC_STEP_HYBRID     2   /* Utils/HybridGradient.m:23-41    Adam, or 100*lr/(fix(t/decay)+1)   */
#define DESC_STEP_EXTERNAL   3   /* params.Gradient is an object the library does not know: the caller
                                    supplies the step of every iteration (the stepping calls below)    */

/* where a per-cycle vector of the stepping calls lives */
#define DESC_MEM_HOST        0
#define DESC_MEM_DEVICE      1   /* device memory on the handle's device                               */

/* where a-1..a-3 (graph, codegree, sampling, mirror maps) are built */
#define DESC_BUILD_HOST      0
#define DESC_BUILD_DEVICE    1

const char* desc_last_error(void);
const char* desc_version(void);
/* number of visible HIP devices, or a negative error code */
int desc_device_count(void);

/* ---------------------------------------------------------------- problem -- */
typedef struct desc_problem {
    int64_t n;              /* number of nodes = max(Ind(:))            DESC_PGD.m:21 */
    int64_t m;              /* number of edges                          DESC_PGD.m:22 */
    const int32_t* ind_i;   /* m, 0-based, ind_i[l] < ind_j[l]          DESC_PGD.m:19 */
    const int32_t* ind_j;   /* m                                        DESC_PGD.m:20 */
    const double* rij;      /* m*9, may be NULL for structure-only calls  DESC_PGD.m:7 */
} desc_problem;

/* A problem resident in the HBM of `device`: edge list, rotations and the CSR index of the graph.  DESC()'s three stages
 * (DESC_PGD -> GCW -> refinement, Algorithms/DESC.m:16-313) and the stand-alone Spectral / CEMP all read the same Ind /
 * RijMat; uploading them once removes two of three 72-B-per-edge host->device copies and CSR passes of a DESC() call.
 * The *_dev entry points below take it in place of a desc_problem.  The caller may free its host arrays afterwards. */
typedef struct desc_device_problem desc_device_problem;   /* opaque, library-owned */
int desc_problem_upload(const desc_problem* prob, int32_t device, desc_device_problem** out);
void desc_problem_free(desc_device_problem* dp);

/* -------------------------------------------------------------- structure -- */
/* The sampled 3-cycle structure of DESC_PGD.m:29-127, sparse.  Cycle c of the
 * l-th edge-with-cycles (edge id pos_edge[l] = (i,j)) lives at
 * cum_ind[l] <= c < cum_ind[l+1] and has third vertex k[c]; inside a segment the
 * k are ascending. */
typedef struct desc_structure desc_structure;   /* opaque, library-owned */

typedef struct desc_structure_view {
    int64_t n, m;
    int64_t m_pos;            /* edges with >=1 triangle                       DESC_PGD.m:50 */
    int64_t m_cycle;          /* sampled cycles in total                       DESC_PGD.m:51 */
    int32_t n_sample;         /* max(ceil(median(codeg>0)/4), n_sample_min)    DESC_PGD.m:43 */
    int32_t max_cnt;          /* longest segment                                             */
    const int32_t* codeg;     /* m      codegree of every edge (0 = no triangle) DESC_PGD.m:29-40 */
    const int32_t* pos_edge;  /* m_pos  CoDeg_pos_ind (0-based edge ids)       DESC_PGD.m:36 */
    const int64_t* cum_ind;   /* m_pos+1                                       DESC_PGD.m:49 */
    const int32_t* k;         /* m_cycle  IJK                                  DESC_PGD.m:93 */
    const int32_t* e_jk;      /* m_cycle  Ind_jk: edge id of {j,k}             DESC_PGD.m:87 */
    const int32_t* e_ki;      /* m_cycle  Ind_ki: edge id of {k,i}             DESC_PGD.m:88 */
    const int32_t* ikj;       /* m_cycle  IKJ: cycle (ik;j), -1 if not sampled DESC_PGD.m:116 */
    const int32_t* jki;       /* m_cycle  JKI: cycle (jk;i), -1 if not sampled DESC_PGD.m:125 */
} desc_structure_view;

/* Build the structure from the edge list.  `datasample` (DESC_PGD.m:84, MATLAB
 * global RNG) is replaced by a counter-based keyed selection: an edge with
 * codeg >= n_sample keeps the n_sample common neighbours k with the smallest
 * desc_sample_key(seed, edge, k).  where = DESC_BUILD_HOST | DESC_BUILD_DEVICE.
 * DESC_BUILD_DEVICE keeps the structure in the HBM of `device` in a lean form (sampled
 * third vertices + per-edge selection thresholds + adjacency); a solver created on the
 * same device lays it out in place without a host round trip.  DESC_ERR_TOO_LARGE means
 * the graph exceeds the device builder's staging budget: use DESC_BUILD_HOST. */
int desc_structure_build(const desc_problem* prob, int32_t n_sample_min, uint64_t seed,
                         int32_t where, int32_t device, desc_structure** out);
/* Adopt a caller-supplied structure (oracle-parity runs; arrays are copied). */
int desc_structure_import(int64_t n, int64_t m, int64_t m_pos, int32_t n_sample,
                          const int32_t* pos_edge, const int64_t* cum_ind,
                          const int32_t* k, const int32_t* e_jk, const int32_t* e_ki,
                          const int32_t* ikj, const int32_t* jki, desc_structure** out);
/* Host view of the full index structure.  For a device-built structure the first call derives
 * e_jk, e_ki and the mirror maps on the device and copies them down (O(m_cycle)); later calls
 * are free.  Not thread-safe per structure; the view stays valid until desc_structure_free.
 * Callers that only need the sizes use desc_structure_sizes, which never touches the device. */
int desc_structure_get(const desc_structure* s, desc_structure_view* view);
/* Sizes and build facts of a structure (DESC_PGD.m:43,50,51) without materialising anything: O(1), no
 * device work, no host copy -- what a binding needs to size the per-cycle in/out vectors
 * (HybridGradient.m_t / v_t) before desc_pgd_create. */
typedef struct desc_structure_info {
    int64_t n, m;
    int64_t m_pos;            /* edges with >=1 triangle                       DESC_PGD.m:50 */
    int64_t m_cycle;          /* sampled cycles in total                       DESC_PGD.m:51 */
    int32_t n_sample;         /* DESC_PGD.m:43 */
    int32_t max_cnt;          /* longest segment */
    int32_t built_where;      /* DESC_BUILD_HOST | DESC_BUILD_DEVICE (imported structures: HOST) */
    int32_t host_resident;    /* 1 when the per-cycle index arrays exist in host memory */
    double  ms_build;         /* wall clock of desc_structure_build, milliseconds */
} desc_structure_info;
int desc_structure_sizes(const desc_structure* s, desc_structure_info* info);
/* Number of times, in this process, a device-built structure was exported to host memory
 * (k_cycle_edges + k_mirror + five O(m_cycle) copies).  Diagnostics: the solver path must not need it. */
int64_t desc_structure_host_exports(void);
void desc_structure_free(desc_structure* s);
uint64_t desc_sample_key(uint64_t seed, uint64_t edge, uint64_t k);

/* ----------------------------------------------------------------- solver -- */
typedef struct desc_params {
    int32_t iters;            /* params.iters                                  DESC_PGD.m:170 */
    int32_t step_kind;        /* DESC_STEP_*                                   DESC_PGD.m:207 */
    double  lr;               /* learning_rate / lr property of the plugin                    */
    double  beta1, beta2;     /* HybridGradient.beta_1/beta_2                                 */
    double  decay_interval;   /* Piecewise/Hybrid decay_interval                              */
    int32_t hybrid_strategy;  /* HybridGradient.strategy: 0 Adam, 1 decayed plain step        */
    int32_t t0;               /* plugin counter t on entry (handle objects keep state)        */
    int32_t patience;         /* 30                                            DESC_PGD.m:180 */
    double  stop_tol;         /* 1e-5                                          DESC_PGD.m:243 */
    int32_t n_sample_min;     /* 30                                            DESC_PGD.m:43  */
    uint64_t seed;            /* sampling seed                                                */
    int32_t verbose;          /* print the reference's progress lines          DESC_PGD.m:241 */
    int32_t device;           /* HIP device ordinal                                           */
    int32_t build_where;      /* DESC_BUILD_*  (one-shot desc_pgd_solve only)                 */
    int32_t check_every;      /* host polls the device stop flag every this many iterations
                                 (0 = library default); results do not depend on it           */
    /* progress lines of DESC_PGD.m:241, streamed while the loop runs (every check_every iterations, 10 by default when
     * a callback or verbose is set): called once per finished iteration, in order, from the thread inside desc_pgd_run /
     * desc_pgd_solve.  NULL with verbose != 0: the reference's fprintf line on stdout.  A MEX shim passes a function that
     * calls mexPrintf. */
    void (*progress)(void* user, int32_t iter, double average_change, double objective);
    void* progress_user;
} desc_params;
void desc_params_default(desc_params* p);

typedef struct desc_result {
    double* s_vec;            /* m        out, caller-allocated: S_vec         DESC_PGD.m:229 */
    double* obj_trace;        /* iters    out or NULL: obj_vals                DESC_PGD.m:233 */
    double* avg_change_trace; /* iters    out or NULL: average_change          DESC_PGD.m:232 */
    double* w;                /* m_cycle  out or NULL: wijk                    DESC_PGD.m:224 */
    double* adam_m;           /* m_cycle  in/out or NULL: HybridGradient.m_t                  */
    double* adam_v;           /* m_cycle  in/out or NULL: HybridGradient.v_t                  */
    int32_t iters_run;        /* iterations executed (early stop, DESC_PGD.m:243-246)         */
    int32_t t_end;            /* plugin counter after the run                                 */
    /* timings, milliseconds */
    double ms_structure;      /* a-1..a-3 build                                               */
    double ms_upload;         /* host -> HBM                                                  */
    double ms_cycle_d;        /* a-4 kernel                                                   */
    double ms_pgd;            /* PGD loop, device time (HIP events)                           */
    double ms_total;          /* wall clock of the call                                       */
} desc_result;

typedef struct desc_pgd desc_pgd;   /* opaque solver handle: one per (problem, device) */

/* Upload problem + structure to HBM and evaluate the cycle inconsistencies
 * S0_long (DESC_PGD.m:129-147).  The structure may be freed afterwards. */
int desc_pgd_create(const desc_problem* prob, const desc_structure* s, int32_t device,
                    desc_pgd** out);
/* the same for a problem already resident in HBM (same device); rank 0 of world 1 = the whole problem */
int desc_pgd_create_dev(const desc_device_problem* dp, const desc_structure* s, int32_t rank, int32_t world, desc_pgd** out);
void desc_pgd_destroy(desc_pgd* h);
/* Full run: init (DESC_PGD.m:148-167) + loop (:182-261) + download. */
int desc_pgd_run(desc_pgd* h, const desc_params* p, desc_result* r);
/* params.make_plots = true (DESC_PGD.m:235-239; the figure of DESC.m:315-344 is drawn from these traces): desc_pgd_run with, after
 * every iteration t, svec_errors[t-1] = mean|err_vec - S_vec| (:236, err_vec = params.ErrVec, m doubles) and the rotation estimate
 * GCW(S_vec) (:237) in R_est_all[(t-1) * 9n ...] (caller-allocated: iters entries / iters * 9n doubles; 3 x 3 x n column-major per
 * iteration).  MSE_means / MSE_medians (:238) = the caller's GlobalSOdCorrectRight(R_est, params.R_orig) of each estimate.
 * dp: the same problem resident on the handle's device.  r->s_vec, obj_trace, avg_change_trace are required.  Entries past
 * r->iters_run are untouched.  r->adam_m / adam_v as in desc_pgd_run. */
int desc_pgd_run_traced(desc_pgd* h, const desc_device_problem* dp, const desc_params* p, const double* err_vec, double gcw_tol,
                        int32_t gcw_max_iters, double* svec_errors, double* R_est_all, desc_result* r);
/* Pieces of desc_pgd_run, for benchmarks and the multi-GPU driver.  All work is
 * enqueued on the handle's stream; _sync waits for it. */
int desc_pgd_reset(desc_pgd* h, const desc_params* p);            /* :148-167                 */
int desc_pgd_iterate(desc_pgd* h, int32_t n_iters);              /* enqueue n_iters sweeps   */
int desc_pgd_iterate_timed(desc_pgd* h, int32_t n_iters, float* ms_total, float* ms_main_kernel_avg);
int desc_pgd_sync(desc_pgd* h);
int desc_pgd_download(desc_pgd* h, desc_result* r);              /* finishes objective trace */
int desc_pgd_get_s0(desc_pgd* h, double* s0 /* m_cycle */);       /* S0_long                  */
int desc_pgd_sizes(const desc_pgd* h, int64_t* m, int64_t* m_pos, int64_t* m_cycle, int32_t* max_cnt);
/* what this handle's layout streams per iteration (bench.py's `floor_bytes`): out[0] = (cycle, endpoint) pairs the mirror-sum pass reads
 * (DESC_PGD.m:185-191: cycles whose mirror was sampled), out[1] = pieces of the band sweep, out[2] = bands, out[3] = CSR entries of band rows
 * staged in the LDS per sweep, out[4] / out[5] = cycles / segments this rank owns; then how the mirror-sum pass runs on this handle (diagnostics):
 * out[6] = lanes per segment of its kernel instance (8 or 16), out[7] = nodes that get a workgroup each, out[8] = nodes it visits (the
 * out[8] - out[7] others: a wave each), out[9] = bits behind the binary point of the 64-bit fixed-point sums, 62 - ceil(log2(max degree + 1));
 * all four are 0 on a handle without the node layout.  Returns how many values were written (<= cap, <= 10). */
int desc_pgd_layout_stats(const desc_pgd* h, int64_t* out, int32_t cap);
/* name of the main-sweep kernel variant chosen for this handle (rocprof cross-reference) */
const char* desc_pgd_kernel_name(const desc_pgd* h);

/* ------------------------------------------- caller-supplied step rule -- */
/* DESC_PGD.m:207 reads  wijk = wijk + params.Gradient.GetStep(grad_long)  for ANY handle object with a GetStep method.  The three
 * classes of Utils/ run inside the sweep (DESC_STEP_CONSTANT / PIECEWISE / HYBRID); every other rule runs through these calls, which
 * cut the iteration at that line: the library computes grad_long, the caller turns it into a step, the library finishes the iteration.
 *     desc_pgd_ext_begin(h, p);                          p->step_kind == DESC_STEP_EXTERNAL; lr, beta*, decay_interval are not read
 *     for (t = 1; t <= p->iters; ++t) {
 *         desc_pgd_ext_grad(h, grad, where);             :185-204 on the current iterate
 *         ... step = GetStep(grad) ...                   :207, the caller's
 *         desc_pgd_ext_apply(h, step, where, &avg, &obj, &stopped);      :207-257
 *         if (stopped) break;                            the patience rule of :243-256 (p->patience, p->stop_tol)
 *     }
 *     desc_pgd_download(h, &r);                          iters_run = steps applied, t_end = p->t0 + iters_run, traces filled
 * grad_long and step hold m_cycle doubles in the reference's cycle order: segment l (the l-th edge with cycles, desc_structure_view
 * pos_edge[l]) at cum_ind[l] .. cum_ind[l+1], its entries in the order of k (IJK) -- whatever layout the handle keeps internally.
 * where = DESC_MEM_HOST: caller host memory, copied down / up (2 x 8 m_cycle bytes per iteration: the slow mode that always works).
 * where = DESC_MEM_DEVICE: device memory of the handle's device; the two passes write / read it in place and no per-cycle data moves
 * between host and device -- only the three scalars do.  The step buffer must be COMPLETE when desc_pgd_ext_apply is called: the
 * library orders its work on the handle's own stream only, so a caller that fills the buffer on another stream synchronises that
 * stream first.  desc_pgd_ext_grad must not be given a buffer the caller still reads on another stream.  Both calls return with
 * the handle's stream synchronised: grad_long is complete, step may be reused.  A non-finite step is the caller's business.
 * Call order: begin, then grad / apply in turns.  apply without a gradient handed out for the iteration, either call before begin,
 * after the stop rule fired or after p->iters steps, and any of the three on a sharded handle (world > 1): DESC_ERR_STATE, nothing is
 * launched.  desc_pgd_reset / desc_pgd_run return the handle to the built-in rules. */
int desc_pgd_ext_begin(desc_pgd* h, const desc_params* p);                                             /* :148-180 */
int desc_pgd_ext_grad(desc_pgd* h, double* grad_long, int32_t where);                                  /* :185-204 */
int desc_pgd_ext_apply(desc_pgd* h, const double* step, int32_t where,                                 /* :207-257 */
                       double* average_change, double* objective, int32_t* stopped);
/* device milliseconds (HIP events) of the last gradient pass, apply pass, and objective + stop rule (tools/stepfn_stages.py) */
int desc_pgd_ext_laps(const desc_pgd* h, double* ms3);

/* ------------------------------------------------------------- multi-GPU -- */
/* One process per GPU.  The edges with cycles (in the library's band-major order) are cut
 * into `world` contiguous ranges of equal cycle count; rank r keeps the per-cycle state
 * (weights, inconsistencies, packed indices) of its range only, and a full replica of the
 * O(m) vectors.  One PGD iteration = desc_pgd_shard_colsum -> reduce-scatter(sum) of T_send
 * into T_recv -> desc_pgd_shard_sweep -> all-gather of sall -> desc_pgd_shard_finish.  The collectives are
 * the caller's (torch.distributed over RCCL in desc_amd/sharded.py); T and sall are device
 * buffers the caller allocates and binds.  All ranks take identical stop decisions because
 * every rank adds the gathered scalar partials in rank order. */
typedef struct desc_shard_info {
    int32_t rank, world;
    int64_t t_len;            /* 8-byte words in T_send = world*xparts*t_part + 1 (mirror sums as fixed-point integers, one block of t_part words per
                                 (exchange part, rank), part-major; last = unused slot) */
    int64_t t_part;           /* words per block: T1 | T2 of the edges of one (rank, part), padded to the largest; T_recv holds xparts blocks */
    int64_t slice_len;        /* doubles per rank in sall: S of the owned edges (padded to the largest shard), then the
                                 workgroup partials (objective, sum |dS|) of the rank's last sweep                      */
    int64_t seg_lo, seg_hi;   /* owned range of edges-with-cycles (library order)             */
    int64_t cyc_lo, cyc_hi;   /* owned range of cycles                                        */
    int64_t m_pos, m_cycle;   /* global counts                                                */
    int32_t xparts;           /* exchange parts per rank (round 4): the reduce-scatter runs part by part -- for c in 0..xparts-1:
                                 reduce_scatter(T_send + c*world*t_part  ->  T_recv + c*t_part, t_part words) -- so that part c + 1 travels
                                 while part c is swept (the fused protocol does; the piecewise calls sweep all parts in desc_pgd_shard_sweep) */
    int32_t reserved;
} desc_shard_info;
int desc_pgd_create_shard(const desc_problem* prob, const desc_structure* s, int32_t device,
                          int32_t rank, int32_t world, desc_pgd** out);
int desc_pgd_shard_info(const desc_pgd* h, desc_shard_info* info);
/* T_send: t_len 8-byte words, zero-initialised by the caller (this rank's partial mirror sums, grouped by
 * owning (part, rank): block b = part*world + rank = [b*t_part, (b+1)*t_part)); the words are 64-bit fixed-point INTEGERS: the caller's
 * reduce-scatter must add them as int64 (ncclInt64 / torch.int64), not as doubles.  T_recv: xparts*t_part words (the caller's
 * reduce-scatter(sum) of every rank's T_send, part by part: see desc_shard_info.xparts); sall: world*slice_len doubles, zero-initialised; all on `device`.
 * All three NULL: the library allocates them itself (the fused protocol below needs no caller buffers).
 * hip_stream: the stream the caller's collectives are ordered on (NULL keeps the handle's own). */
int desc_pgd_shard_bind(desc_pgd* h, double* T_send, double* T_recv, double* sall, void* hip_stream);
/* Piecewise protocol (one call per step, the caller runs the collectives in between; kept for drivers that own
 * the communication, e.g. torch.distributed with a backend other than RCCL, and for single-GPU emulation tests). */
int desc_pgd_shard_colsum(desc_pgd* h);
int desc_pgd_shard_sweep(desc_pgd* h);
/* initial: 0 = after an iteration's all-gather; 1 = after reset, before the first all-gather (no-op: the reset
 * already put the initial S of the owned edges into the slice); 2 = unpack the initial S_vec (after that all-gather). */
int desc_pgd_shard_finish(desc_pgd* h, int32_t initial);
/* objective of the last iterate: phase 0 puts this rank's partials into its slice (then all-gather sall),
 * phase 1 adds the partials of all ranks and runs the stop rule for the last iteration. */
int desc_pgd_shard_objective(desc_pgd* h, int32_t phase);

/* Fused protocol: the library enqueues whole iterations itself -- column sums, reduce-scatter, sweep, all-gather,
 * unpack + stop rule -- on two streams, so that the all-gather of S_vec and its unpacking overlap the next
 * iteration's column-sum pass (which needs only the weights).  The collectives are the caller's: two function
 * pointers with the signatures of RCCL's ncclReduceScatter / ncclAllGather (hipStream_t stream; the reduce-scatter is
 * called with datatype 4 = ncclInt64 and op 0 = ncclSum -- the mirror sums of DESC_PGD.m:189-190 travel as 64-bit fixed-point
 * integers, whose sum does not depend on the order the ranks' parts are added in --, the all-gather with datatype 8 =
 * ncclDouble) and the communicator they take; a binding passes the addresses of the RCCL
 * symbols of the process (desc_amd/sharded.py: the librccl.so PyTorch ships, communicator created with
 * ncclCommInitRank from an id broadcast over torch.distributed) or its own trampolines.  world == 1: both may
 * be NULL.  Nothing in the reference corresponds to this (it is single-process MATLAB). */
typedef struct desc_collectives {
    void* comm;               /* ncclComm_t (opaque to the library) */
    int (*reduce_scatter)(const void* sendbuff, void* recvbuff, size_t recvcount, int datatype, int op, void* comm, void* stream);
    int (*all_gather)(const void* sendbuff, void* recvbuff, size_t sendcount, int datatype, void* comm, void* stream);
} desc_collectives;
int desc_pgd_shard_set_collectives(desc_pgd* h, const desc_collectives* c);
int desc_pgd_shard_start(desc_pgd* h, const desc_params* p);          /* reset + initial exchange of S_vec        */
int desc_pgd_shard_iterate(desc_pgd* h, int32_t n_iters);             /* enqueue n_iters iterations               */
/* start + iterate (the stop flag is polled every p->check_every iterations; identical on all ranks) + objective of
 * the last iterate + download (S_vec, traces; per-cycle outputs are not gathered across ranks). */
int desc_pgd_shard_run(desc_pgd* h, const desc_params* p, desc_result* r);
/* *stopped = 1 once the device-side patience rule (DESC_PGD.m:243-246) has fired; waits for
 * the handle's stream. */
int desc_pgd_stopped(desc_pgd* h, int32_t* stopped);

/* ------------------------------------------------- Spectral / GCW (next row f-1) -- */
/* Top-3 eigenvectors ('la') of the 3n x 3n block connection matrix + per-node projection onto
 * SO(3).  weights == NULL, normalize_rows == 0: Algorithms/Spectral.m:18-46.
 * weights[l] = 1/(S_vec[l]^1.5 + 1e-8), normalize_rows == 1: Utils/GCW.m:9-36 (the matrix
 * D^-1*W .* Rij_blk; iterated in its symmetric similar form, eigenvectors mapped back and
 * re-normalised).  R_out: n*9 doubles, 3x3xn in MATLAB column-major order.  Rotations are
 * defined up to one global right rotation (compare after Utils/Rotation_Alignment.m). */
typedef struct desc_spectral_info {
    int32_t iters;            /* outer (filter + Rayleigh-Ritz) steps              */
    int32_t products;         /* block matrix products (3n x 6 each)               */
    int32_t converged;        /* residual <= tol reached                           */
    int32_t reserved;         /* desc_gcw_batch_run: the kernel that solved the problem (DESC_GCW_EIG_LDS or _STREAMED); else 0 */
    double  residual;         /* max relative residual of the three Ritz pairs     */
    double  eigenvalues[3];   /* the three largest eigenvalues                     */
    double  ms_total;
} desc_spectral_info;
int desc_spectral_run(const desc_problem* prob, const double* weights, int32_t normalize_rows, double tol,
                      int32_t max_iters, int32_t device, double* R_out, desc_spectral_info* info);
int desc_spectral_run_dev(const desc_device_problem* dp, const double* weights, int32_t normalize_rows, double tol,
                          int32_t max_iters, double* R_out, desc_spectral_info* info);
/* R_est = GCW(Ind, AdjMat, RijMat, SVec) -- Utils/GCW.m:9-36 -- with the weights 1/(SVec.^1.5 + 1e-8) (GCW.m:20) and the
 * weighted degrees formed on the device from s_vec (m doubles, host). */
int desc_gcw_run_dev(const desc_device_problem* dp, const double* s_vec, double tol, int32_t max_iters, double* R_out,
                     desc_spectral_info* info);

/* ------------------------------------------------------------ CEMP (next row f-2) -- */
/* SVec = CEMP(Ind, RijMat, CEMP_parameters) -- Algorithms/CEMP.m:24-132.  beta[0..n_beta-1] =
 * CEMP_parameters.reweighting (missing entries repeat the last one, CEMP.m:30-34), max_iter =
 * .max_iter, nsample = .nsample (cycles per edge, sampled with replacement, CEMP.m:64; MATLAB's
 * RNG is replaced by CoInd[desc_sample_key(seed, edge, t) mod codeg]).  s_vec: m doubles out. */
int desc_cemp_run(const desc_problem* prob, const double* beta, int32_t n_beta, int32_t max_iter, int32_t nsample,
                  uint64_t seed, int32_t device, double* s_vec, double* ms_total);
int desc_cemp_run_dev(const desc_device_problem* dp, const double* beta, int32_t n_beta, int32_t max_iter, int32_t nsample,
                      uint64_t seed, double* s_vec, double* ms_total);

/* ----------------------------------------- DESC refinement tail (next row f-3) -- */
/* Reweighted Lie-algebraic averaging, Algorithms/DESC.m:265-313 with Utils/Weighted_LAA.m,
 * Build_Amatrix.m, R2Q.m, q2R.m.  s_vec: m (the PGD output), R_init: n*9 (3x3xn column-major, the
 * GCW output, DESC.m:263), R_out: n*9.  stop_threshold <= 0 -> 1e-3, max_iters <= 0 -> 100
 * (DESC.m:272).  MATLAB's sparse-QR least squares is replaced by f64 PCG on the normal equations; the
 * weights span 1e-4..1e4 (DESC.m:279-282), squared in the normal equations, so a solve may stop at its
 * iteration cap: info->cg_unconverged / cg_residual say so, and a warning is printed to stderr. */
typedef struct desc_refine_info {
    int32_t iters;            /* refinement steps executed                                     */
    int32_t cg_iters;         /* conjugate-gradient steps in total                             */
    int32_t verbose;          /* in: print the reference's "Iter %d: ||dR||= %f" lines          */
    int32_t cg_unconverged;   /* refinement steps whose PCG solve stopped at its iteration cap
                                 before reaching |r| <= 1e-13 |b| (0 = every solve converged)   */
    double  score;            /* last mean rotation update (Weighted_LAA.m:40)                 */
    double  ms_total;
    double  cg_residual;      /* largest relative residual |r|/|b| left by any of the solves   */
} desc_refine_info;
int desc_refine_run(const desc_problem* prob, const double* s_vec, const double* R_init, double stop_threshold,
                    int32_t max_iters, int32_t device, double* R_out, desc_refine_info* info);
int desc_refine_run_dev(const desc_device_problem* dp, const double* s_vec, const double* R_init, double stop_threshold,
                        int32_t max_iters, double* R_out, desc_refine_info* info);

/* ------------------------------------------------------------- MPLS / CEMP+MST -- */
/* R_est = MST step of Algorithms/MPLS.m:160-193: the minimum spanning tree of the graph with edge weights s_vec + 1 (:162 -- NOT
 * Utils/MST.m, whose sparse() call drops the edges with s_vec == 0), rooted at node 1 with R_1 = I; a leaf reached through edge e
 * gets R_e * R_root when it is e's smaller endpoint, R_e' * R_root otherwise (:178-193).  Edge order: the double fl(s_vec[e] + 1.0),
 * ties broken by the edge index e (the (i, j)-sorted order), so the tree is unique; MATLAB's minspantree (:166-168) does not document
 * its tie rule, and with distinct keys both trees coincide.  R_out: n*9 doubles; tree_edges (nullable): the n - 1 tree edges'
 * indices, ascending.  A graph that is not connected -- two pieces, or a node id in 1..n that no edge touches -- is refused with
 * DESC_ERR_INVALID and the number of components in desc_last_error() (the reference loops for ever there, :178). */
int desc_mst_run(const desc_problem* prob, const double* s_vec, int32_t device, double* R_out, int32_t* tree_edges);
int desc_mst_run_dev(const desc_device_problem* dp, const double* s_vec, double* R_out, int32_t* tree_edges);

/* [R_est, R_init] = MPLS(Ind, RijMat, CEMP_parameters, MPLS_parameters) -- Algorithms/MPLS.m:31-257.  CEMP (:65-158, the text of
 * CEMP.m:36-132, sampled as desc_cemp_run does) -> the MST initialisation above (:160-193) -> the MPLS loop (:196-249): Weighted_LAA
 * (as desc_refine_run), residuals r = |A W(2:end,2:4) - B|/pi (:221-222), the cycle step h_ij = sum w .* S0Mat with
 * w = exp(-beta_t (r_ik + r_jk)) normalised per edge over CEMP's own samples (:223-237), RH = (1 - alpha_t) r + alpha_t h (:240),
 * weights min(1/RH^0.75, 1e4), 1e-4 where RH > quantile(RH, tau_t) (:241-245); initial weights min(1/SVec^0.75, 1e4) (:210-213);
 * while score > stop_threshold && Iteration < max_iter (:218).  beta / tau / alpha are indexed by Iteration and padded with their
 * last entry (:47-63), as is cemp_beta (:37-42).  As in the reference, an edge without a 3-cycle is not reset in the loop (:239 is
 * commented out): its cycle product is the zero matrix, so its S0 is |acos(-1/2)|/pi = 2/3, its weights 1/nsample, its h 2/3.
 * CEMP's samples and S0Mat stay resident for the whole loop (m_pos * nsample doubles; m_pos * nsample must stay below 2^31, else
 * DESC_ERR_TOO_LARGE).  R_est, R_init (nullable): n*9 doubles; s_vec_out (nullable): CEMP's SVec, m doubles. */
typedef struct desc_mpls_params {
    const double* cemp_beta;  /* CEMP_parameters.reweighting                         MPLS.m:35 */
    int32_t n_cemp_beta;
    int32_t cemp_max_iter;    /* CEMP_parameters.max_iter                            MPLS.m:34 */
    int32_t nsample;          /* CEMP_parameters.nsample                             MPLS.m:36 */
    int32_t verbose;          /* print the reference's disp / fprintf lines                    */
    uint64_t seed;            /* cycle-sampling key (MATLAB: global RNG, MPLS.m:93)            */
    double stop_threshold;    /* MPLS_parameters.stop_threshold                      MPLS.m:45 */
    int32_t max_iter;         /* MPLS_parameters.max_iter                            MPLS.m:46 */
    int32_t n_beta;
    const double* beta;       /* MPLS_parameters.reweighting                         MPLS.m:47 */
    const double* tau;        /* MPLS_parameters.thresholding                        MPLS.m:53 */
    const double* alpha;      /* MPLS_parameters.cycle_info_ratio                    MPLS.m:59 */
    int32_t n_tau;
    int32_t n_alpha;
} desc_mpls_params;
typedef struct desc_mpls_info {
    int32_t iters;            /* MPLS iterations executed (Iteration - 1)                      */
    int32_t cg_iters;         /* conjugate-gradient steps in total                             */
    int32_t cg_unconverged;   /* Weighted_LAA solves that stopped at the PCG iteration cap     */
    int32_t reserved;
    int64_t m_pos;            /* edges with a 3-cycle                                          */
    double  score;            /* last mean rotation update (Weighted_LAA.m:40)                 */
    double  cg_residual;      /* largest relative residual |r|/|b| left by any solve           */
    double  ms_cemp, ms_mst, ms_loop, ms_total;
} desc_mpls_info;
int desc_mpls_run(const desc_problem* prob, const desc_mpls_params* params, int32_t device, double* R_est, double* R_init,
                  double* s_vec_out, desc_mpls_info* info);
int desc_mpls_run_dev(const desc_device_problem* dp, const desc_mpls_params* params, double* R_est, double* R_init,
                      double* s_vec_out, desc_mpls_info* info);

/* ------------------------------------------------------------- IRLS_GM / IRLS_L12 -- */
/* R = IRLS_GM(RijMat, Ind) / IRLS_L12(RijMat, Ind) -- Algorithms/IRLS_GM.m, IRLS_L12.m (Chatterjee & Govindu).  Five stages:
 *   1. RR = permute(RijMat, [2,1,3]), I = Ind' (:52-53).
 *   2. the largest connected component (:65-67) of the graph on nodes 1..n = max(Ind(:)) (a node id no edge touches is a component of
 *      its own).  Of several of maximal size the one holding the smallest node id is taken -- an assumption about how graphconncomp
 *      numbers undirected components, which does not matter when the sizes differ.  Its nodes are renumbered in increasing id order,
 *      its edges keep their order; every node outside it gets NaN in R_out (:94).  With R_init, the component's rows are used (the
 *      reference passes the full-size Rinit to the sub-problem unindexed and fails there).
 *   3. per edge, all of them (:82-93): det(RR) <= 0 is an error; an error too when ALL three singular values deviate from 1 by >= 0.1
 *      (MATLAB's `if` on a vector), a warning when all three deviate by >= 0.01 (the count is printed to stderr and returned);
 *      then RR = U * round(S) * V'.  The error names the smallest failing row of the caller's Ind (1-based, via `order`).
 *   4. BoxMedianSO3Graph(RR, I, Rinit, max_iter_l1) (Utils/BoxMedianSO3Graph.m): Q from R_init, or from the spanning-tree pass
 *      (:79-114) over the edges in the caller's row order; then while score >= 1e-3 (with L1Step = 2 the reference's L1Step branch
 *      never fires; it is restated), per coordinate an l1-magic primal-dual solve of min |B(:,c) - A x|_1 (l1decode_pd, :245-360)
 *      with pdtol = eps and at most L1Step steps; score = max_v |W_v| (:173); R_l1 = real(q2R(Q)).
 *   5. RobustMeanSO3Graph (GM, weights SIGMA/(|E|^2 + SIGMA^2), SIGMA in radians) or L12 (weights min(|E|^-0.75, 1e4)) from
 *      Q = R2Q(R_l1): Weighted_LAA steps with E = A W - B of the solved W, while score = sum |W_v| / n > 1e-3 (:130-176).
 * Deviations: l1decode_pd's dense LU of H11p = A' diag(sigx) A is a Jacobi-preconditioned CG on the device (one weight vector per
 * coordinate, |r| <= 1e-13 |b|); LAPACK's rcond test (hcond < 1e-14, "Matrix ill-conditioned") becomes a CG breakdown -- a
 * non-finite value or p'Hp <= 0 -- and a solve that stops at its iteration cap is counted in cg_unconverged and warned about.  The
 * weighted least squares of stage 5 are the normal equations by PCG, as desc_refine_run.  Input rules as elsewhere: 1-based,
 * Ind(:,1) < Ind(:,2), no duplicate edge (the problem's edges sorted by (i, j); `order` gives the caller's row of each).
 * R_out: n*9 doubles; R_l1 (nullable): the stage-4 estimate, n*9 doubles, NaN outside the component. */
enum { DESC_IRLS_GM = 0, DESC_IRLS_L12 = 1 };
typedef struct desc_irls_params {
    int32_t mode;             /* DESC_IRLS_GM (RobustMeanSO3Graph) or DESC_IRLS_L12 (L12)                */
    int32_t max_iter_l1;      /* MaxIterations(1); <= 0: 10                              IRLS_GM.m:59 */
    int32_t max_iter_irls;    /* MaxIterations(2); <= 0: 100                             IRLS_GM.m:59 */
    int32_t verbose;          /* print the reference's fprintf / disp lines and early-return messages     */
    double sigma_deg;         /* SIGMA in degrees; <= 0: 5 (GM only)                     IRLS_GM.m:58 */
    const double* R_init;     /* nullable: Rinit, n*9 doubles (3x3xn, column-major)      IRLS_GM.m:57 */
    const int32_t* order;     /* nullable: order[e] = the caller's 0-based row of edge e (a permutation of 0..m-1): the
                                 row order of the tree pass and of the error message; NULL = the edge order itself  */
} desc_irls_params;
typedef struct desc_irls_info {
    int64_t comp_nodes;       /* nodes and edges of the largest component                               */
    int64_t comp_edges;
    int32_t l1_iters;         /* BoxMedianSO3Graph iterations                                           */
    int32_t irls_iters;       /* RobustMeanSO3Graph / L12 iterations                                    */
    double  l1_score;         /* last L1 score: max_v |W_v|                                             */
    double  irls_score;       /* last IRLS score: sum_v |W_v| / n                                       */
    int32_t pd_steps;         /* primal-dual steps taken, all coordinates and iterations                */
    int32_t pd_ill;           /* l1decode_pd returns "Matrix ill-conditioned" (a CG breakdown here)     */
    int32_t pd_stuck;         /* l1decode_pd returns "Stuck backtracking"                               */
    int32_t warned_edges;     /* edges whose three singular values all deviate by >= 0.01               */
    int32_t cg_iters_l1;      /* CG steps of the batched Newton solves, each rounded up to the probe interval 5 */
    int32_t cg_iters_irls;    /* CG steps of the Weighted_LAA solves, each rounded up to laa_step's probe interval 25 */
    int32_t cg_unconverged;   /* solves (both stages) that stopped at the CG iteration cap              */
    int32_t pd_solves;        /* batched Newton solves of the L1 stage (one CG for the three coordinates) */
    double  cg_residual;      /* largest relative residual |r|/|b| left by any solve                    */
    double  ms_project, ms_components, ms_tree, ms_l1, ms_l1_pcg, ms_irls, ms_total;
} desc_irls_info;
int desc_irls_run(const desc_problem* prob, const desc_irls_params* params, int32_t device, double* R_out, double* R_l1,
                  desc_irls_info* info);
int desc_irls_run_dev(const desc_device_problem* dp, const desc_irls_params* params, double* R_out, double* R_l1,
                      desc_irls_info* info);

/* ------------------------------------------------------------------ linprog_sij -- */
/* S_vec of Algorithms/linprog_sij.m:16-139: the LP  min sum_l s_l  s.t.  |s_l - d_lt| <= s_ik + s_jk  on nsample sampled 3-cycles per edge
 * with cycles ("pos" edges, ascending edge order), 0 <= s <= 1; edges without a cycle keep 1 (:104).  nsample = 0: the rule
 * max(ceil(median(codeg of pos edges) / 4), 30) (:43, = desc_structure_info.n_sample of the same graph).  The t-th sample of edge l is
 * CoInd[desc_sample_key(seed, l, t) mod codeg] (desc_cemp_run's rule, in place of datasample at :68).  Rows of cycle (l, t) with
 * d = S0Mat(t, l), a = {i,k}, b = {j,k}:  s_l - s_a - s_b <= d  and  -s_l - s_a - s_b <= -d.  One deliberate departure: :84-85 index
 * Ind_i(l) / Ind_j(l) with l running over the pos edges; the edge's own endpoints are used (equal whenever every edge lies on a triangle).
 * Solver (lp.hip): matrix-free PDHG on the device in f64,  x+ = clip(x - tau o (1 + K'y), 0, 1),  y+ = max(y + sigma o (K(2x+ - x) - b), 0),
 * tau_l = 1 / (w sum_r |K_rl|), sigma_r = w / 3, primal weight w = 1 until the first restart; restarts to the running average as in PDLP.
 * Every check_every steps:  viol = max_r max((Kx - b)_r, 0),  P = sum x,  D = -b'y + sum_l min(0, 1 + (K'y)_l) (<= the optimum for every
 * y >= 0); stop when viol <= tol and P - D <= tol (1 + |P| + |D|).  Reaching max_iter is no error: converged = 0 and a warning on stderr.
 * restart = 0 and tol = 0: exactly max_iter plain steps from x = 0, y = 0 with w = 1.  Two runs on the same input return the same bits.
 * s_vec: m doubles.  y (nullable): 2 nsample m_pos doubles, [pos edge][t][row 1, row 2].  k_out (nullable): nsample m_pos sampled third
 * nodes, 1-based, [pos edge][t].  A call with max_iter = 0 and y = k_out = NULL takes no step and only fills info (nsample, m_pos, rows):
 * what a caller needs to size y, k_out and params->pos_out.
 * Size limits: 2 nsample m_pos < 2^31 (DESC_ERR_TOO_LARGE).  The cycles are sampled on the device while no edge has more than 4096
 * common neighbours; beyond that the host sampler takes over -- same keyed rule, same samples -- but only for an explicit nsample > 0.
 * With nsample = 0 (the rule, which belongs to the device sampler) such a graph is refused: DESC_ERR_TOO_LARGE, "an edge has <c> common
 * neighbours".  Pass nsample to solve it. */
typedef struct desc_lp_params {
    int32_t nsample;          /* 0: the rule of :43                                            */
    int32_t check_every;      /* steps between two evaluations of the certificates; 0: 64      */
    uint64_t seed;            /* cycle-sampling key                                            */
    double  tol;              /* 1e-4                                                          */
    int32_t max_iter;         /* 200000                                                        */
    int32_t restart;          /* 1: averages, restarts and primal weight; 0: the plain recurrence */
    int32_t verbose;          /* 1: one line per check; 2: also hipEvent laps of the two kernels (every step synchronises) */
    int32_t reserved;
    int32_t* pos_out;         /* nullable: receives the m_pos pos edges (0-based edge ids, ascending): the LP's variables */
} desc_lp_params;             /* 48 bytes */
void desc_lp_params_default(desc_lp_params* p);
typedef struct desc_lp_info {
    int32_t nsample, iters, restarts, converged;
    int64_t m_pos, rows;      /* variables; inequality rows = 2 nsample m_pos                  */
    double  viol, pobj, dobj; /* the certificates of what was returned                         */
    double  ms_samples;       /* samples + S0Mat                                               */
    double  ms_transpose;     /* the transposed incidence                                      */
    double  ms_loop;
    double  ms_col, ms_row;   /* verbose = 2: mean per step of the two kernels                 */
    double  ms_total;
} desc_lp_info;               /* 104 bytes */
int desc_lp_sij_run(const desc_problem* prob, const desc_lp_params* params, int32_t device, double* s_vec, double* y, int32_t* k_out,
                    desc_lp_info* info);
int desc_lp_sij_run_dev(const desc_device_problem* dp, const desc_lp_params* params, double* s_vec, double* y, int32_t* k_out,
                        desc_lp_info* info);

/* ------------------------------------------------- many small problems in one pass -- */
/* B independent problems (the Monte-Carlo studies of the paper: graphs of 100-200 nodes, many trials) share one set of device arrays and
 * ONE sweep launch per iteration.  Problem b returns what desc_pgd_solve(probs[b], p) returns with seed seeds[b] (p->seed when seeds is
 * NULL) and the host builder: its own n_sample, its cycles sampled with its LOCAL edge and node ids, its own S0_long, traces, patience
 * rule and stop iteration.  A problem that stops is frozen while the others run on; the call ends when all have stopped or after
 * p->iters iterations.  The result of a problem is bitwise independent of the batch around it (position, neighbours, batch size): how
 * its segments are cut into workgroups and the order its partial sums are added in depend on that problem alone; no floating-point
 * atomics anywhere.  All problems sit behind one another: edges of problem b at edge_off[b] .. edge_off[b+1] of every per-edge vector,
 * its cycles at cycle_off[b] .. cycle_off[b+1] of every per-cycle vector (the problem's own cycle order).
 * desc_pgd_batch_create: validates, builds the structures on min(count, 16) host threads, refuses -- all before any device work, naming
 * the problem -- a problem whose n_sample exceeds 64 (DESC_ERR_INVALID: solve it with desc_pgd_solve) and totals of m_cycle >= 2^31 - 1
 * or m >= 2^30 (DESC_ERR_TOO_LARGE); then uploads and evaluates S0_long of the whole batch.  p: n_sample_min, seed and device are read
 * (p->build_where is NOT: the builder of a batch is chosen by desc_pgd_batch_create_where).
 * count == 0 is legal.  Step rules: DESC_STEP_CONSTANT / PIECEWISE / HYBRID, one desc_params for the whole batch.
 *
 * desc_pgd_batch_create_where(.., where, ..): where = DESC_BUILD_HOST is desc_pgd_batch_create.  where = DESC_BUILD_DEVICE makes the
 * same index arrays, element for element, on the device: the host validates and builds the CSR of every problem (O(m); no triangle
 * is touched on the host), five launches for the whole batch count the codegrees, plan, compact, sample and mirror, and the only
 * read-back is one record per problem.  Everything downstream (S0_long, the sweep, the stop rule, S_vec, w, the traces) is bit for bit
 * what the host builder gives.  It refuses what the host builder refuses, with the same code and the same "problem b"; n_sample > 64
 * and the 2^31 - 1 total are known only after that read-back and are refused there, after device work: the handle is then closed and
 * nothing is left allocated.  Two cases make the whole batch fall back to the host builder, silently and without failing: a problem
 * with a CSR row above desc_cemp_batch_max_degree(), and a problem with a codegree above desc_pgd_batch_max_codeg() (what the sampling
 * kernel stages in the 64 KiB of LDS a launch may declare).  desc_pgd_batch_built_where tells which builder made the handle.  Any other
 * value of where: DESC_ERR_INVALID.  DESC_DEBUG_EXACT_SELECT=1 (read at create) forces the tie-safe exact ranking for every edge. */
typedef struct desc_pgd_batch desc_pgd_batch;   /* opaque */
typedef struct desc_batch_result {
    double* s_vec;            /* edge_off[count]   out: S_vec of every problem                                  */
    double* obj_trace;        /* count * p->iters  out or NULL: row b = obj_vals of problem b; entries past
                                 iters_run[b] are zero                                                          */
    double* avg_change_trace; /* count * p->iters  out or NULL: average_change, likewise                        */
    double* w;                /* cycle_off[count]  out or NULL: wijk                                            */
    double* adam_m;           /* cycle_off[count]  in/out or NULL: HybridGradient.m_t (read when p->t0 > 0)     */
    double* adam_v;           /* cycle_off[count]  in/out or NULL: HybridGradient.v_t                           */
    int32_t* iters_run;       /* count             out: iterations problem b executed                           */
    int32_t* t_end;           /* count             out or NULL: plugin counter of problem b after the run       */
    double ms_structure;      /* wall clock of create up to the point where the index arrays are on the device (either builder) */
    double ms_upload;         /* the remainder of the set-up: the rotations, the small tables, the state buffers  */
    double ms_cycle_d;        /* S0_long kernel                                                                 */
    double ms_pgd;            /* PGD loop, device time (HIP events)                                             */
    double ms_total;          /* wall clock of desc_pgd_batch_run                                               */
} desc_batch_result;          /* 104 bytes */
int desc_pgd_batch_create(const desc_problem* probs, int32_t count, const desc_params* p, const uint64_t* seeds /* count, nullable */,
                          desc_pgd_batch** out);
int desc_pgd_batch_create_where(const desc_problem* probs, int32_t count, const desc_params* p, const uint64_t* seeds /* count, nullable */,
                                int32_t where /* DESC_BUILD_HOST | DESC_BUILD_DEVICE */, desc_pgd_batch** out);
int32_t desc_pgd_batch_built_where(const desc_pgd_batch* h);      /* DESC_BUILD_HOST | DESC_BUILD_DEVICE: the builder that made the handle */
int32_t desc_pgd_batch_max_codeg(void);                           /* the largest codegree the device builder's sampling kernel stages */
/* device time (ms, HIP events) of the device builder's five launches: codegrees, plan, compaction, sampling, mirror maps; zeros for a
 * host-built handle */
int desc_pgd_batch_build_laps(const desc_pgd_batch* h, double* ms /* 5 */);
/* the plan rule of the device builder on a histogram of codegrees (hist[c], c = 0 .. n), for tests; no device.
 * out: m_pos, max_codeg, n_sample, m_cycle, max_cnt */
int desc_test_batch_plan(const int32_t* hist, int32_t n, int32_t n_sample_min, int64_t* out /* 5 */);
/* count (nullable), edge_off[count+1], cycle_off[count+1], n_sample[count] (each nullable): what a binding needs to size its buffers */
int desc_pgd_batch_sizes(const desc_pgd_batch* h, int32_t* count, int64_t* edge_off, int64_t* cycle_off, int32_t* n_sample);
/* the structure of problem b, local ids (parity tests); the view stays valid until desc_pgd_batch_destroy.  On a device-built handle the
 * first request downloads the index arrays once and fills a host-resident structure per problem; the plain run never does. */
int desc_pgd_batch_get_structure(const desc_pgd_batch* h, int32_t b, desc_structure_view* view);
int desc_pgd_batch_get_s0(desc_pgd_batch* h, double* s0 /* cycle_off[count] */);
/* init + loop + download.  p->check_every: the host reads one "problems still running" word every this many iterations (0: 32);
 * results do not depend on it.  progress / verbose are not used. */
int desc_pgd_batch_run(desc_pgd_batch* h, const desc_params* p, desc_batch_result* r);
void desc_pgd_batch_destroy(desc_pgd_batch* h);
/* Host part of the set-up (no device): the structures of `count` problems behind one another, per-problem edge / cycle / segment offsets
 * added to pos_edge, cum, e_jk, e_ki, ikj, jki (-1 stays -1).  edge_off, cycle_off, seg_off: count + 1 entries each; cum: seg_off[count] + 1
 * entries; any of the seven arrays may be NULL (offsets only: what a caller needs to size the others). */
int desc_pgd_batch_concat(const desc_structure* const* s, int32_t count, int64_t* edge_off, int64_t* cycle_off, int64_t* seg_off,
                          int32_t* pos_edge, int32_t* cum, int32_t* e_jk, int32_t* e_ki, int32_t* ikj, int32_t* jki);

/* Spectral / GCW for B independent small problems in ONE launch: the rotation step behind desc_pgd_batch_* (S_vec -> R_est, GCW.m:9-36 /
 * DESC.m:263).  One workgroup per problem runs the whole Chebyshev-filtered subspace iteration of desc_spectral_run on the chip (its
 * 3n x 6 blocks in LDS, the 6x6 Jacobi and the Cholesky coefficients inside the kernel, no host round trip); the tail (back-scaling,
 * unit columns, det sign, per-node projection onto SO(3)) runs per problem on host threads.  Problem b's result is bitwise independent
 * of the batch around it (position, neighbours, batch size, the LDS size of the launch).  It agrees with desc_spectral_run /
 * desc_gcw_run_dev to the accuracy of the eigen-solve, not bit for bit: the Gram sums are taken in another (fixed) order.
 * desc_gcw_batch_max_n: the largest n whose blocks fit the 160 KiB of LDS a workgroup may declare (278).
 * desc_gcw_batch_create: validates every problem and refuses -- before any device work, naming the problem -- an empty edge list and
 * n > desc_gcw_batch_max_n() (DESC_ERR_INVALID: solve it with GCW / DESC_init); builds the per-problem CSR (local ids) and uploads
 * rotations and indices in one copy each.  count == 0 is legal.  The handle may be run any number of times.
 * desc_gcw_batch_create_where: create with a choice of where the four blocks live.  DESC_GCW_EIG_LDS is desc_gcw_batch_create.
 * DESC_GCW_EIG_STREAMED solves every problem with the streamed kernel: the blocks in a per-problem global workspace (72 n doubles,
 * allocated only where a problem streams), one staging block in LDS for the source of the current product; the cap is
 * desc_gcw_batch_streamed_max_n() (1112).  DESC_GCW_EIG_AUTO gives a problem of n <= desc_gcw_batch_max_n() to the LDS kernel and a
 * larger one to the streamed kernel -- by its own n alone, at most two launches on the handle's stream, both inside ms_eig.  The
 * arithmetic is the same text in the same order: a problem gets the same bits from either kernel.  Refused before any device work
 * (DESC_ERR_INVALID): an eig that is none of the three, and n above the cap of the mode, naming the problem.  infos[b].reserved of
 * desc_gcw_batch_run says which kernel solved problem b.
 * desc_gcw_batch_sizes: node_off[count+1], edge_off[count+1] (each nullable).
 * desc_gcw_batch_csr: the host part of create alone (no device): rowptr (problem b's n_b + 1 entries at node_off[b] + b), adj and adj_eid
 * (its 2 m_b entries at 2 edge_off[b]; local node / edge ids); the three arrays are nullable (offsets only, to size them).
 * desc_gcw_batch_run: s_vec = the edge_off[count] concatenated S_vec in the library's edge order: GCW mode (weights 1/(S^1.5 + 1e-8)
 * formed on the device, rows normalised); s_vec NULL and weights NULL: Spectral mode with normalize_rows == 0; s_vec NULL and weights
 * set: host weights as desc_spectral_run.  A negative or non-finite S_vec entry (or weight) is refused, naming the problem and the node.
 * R_out: problem b's 3x3xn_b column-major blocks at 9 * node_off[b]; infos: count entries (ms_total = the call's).  tol <= 0: 1e-13,
 * max_iters <= 0: 500.  A problem that does not converge reports converged = 0 and the rotations of its last basis. */
typedef struct desc_gcw_batch desc_gcw_batch;   /* opaque */
typedef struct desc_gcw_batch_timings {
    double ms_structure;      /* validation + per-problem CSR (wall clock of create's host part)   */
    double ms_upload;         /* host -> HBM (create)                                               */
    double ms_eig;            /* the eigen-solve launch, device time (HIP events)                   */
    double ms_project;        /* the tail on host threads                                           */
    double ms_total;          /* wall clock of desc_gcw_batch_run                                   */
} desc_gcw_batch_timings;     /* 40 bytes */
#define DESC_GCW_EIG_LDS       0
#define DESC_GCW_EIG_STREAMED  1
#define DESC_GCW_EIG_AUTO      2
int32_t desc_gcw_batch_max_n(void);
int32_t desc_gcw_batch_streamed_max_n(void);
int desc_gcw_batch_create(const desc_problem* probs, int32_t count, int32_t device, desc_gcw_batch** out);
int desc_gcw_batch_create_where(const desc_problem* probs, int32_t count, int32_t device, int32_t eig, desc_gcw_batch** out);
int desc_gcw_batch_sizes(const desc_gcw_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off);
int desc_gcw_batch_csr(const desc_problem* probs, int32_t count, int64_t* node_off, int64_t* edge_off, int32_t* rowptr, int32_t* adj,
                       int32_t* adj_eid);
int desc_gcw_batch_run(desc_gcw_batch* h, const double* s_vec, const double* weights, int32_t normalize_rows, double tol, int32_t max_iters,
                       double* R_out, desc_spectral_info* infos, desc_gcw_batch_timings* timings /* nullable */);
void desc_gcw_batch_destroy(desc_gcw_batch* h);

/* CEMP (Algorithms/CEMP.m:24-132) for B independent small problems in one GPU pass: the baseline next to desc_pgd_batch_*.  The edge
 * lists lie behind one another; ONE launch in create samples the 3-cycles and evaluates S0 and the initial means for the whole batch
 * (CEMP.m:44-103: one wave per edge intersects the two CSR rows in ascending k, draws sample t as
 * CoInd[desc_sample_key(seed_b, local edge id, t) mod codeg] -- desc_cemp_run's rule -- and keeps nsample slots per edge of the batch, with
 * or without cycles: no compaction, no host round trip), and every round (:107-128) is one launch for the whole batch.
 * Problem b's S_vec is bit for bit what desc_cemp_run gives for it with its seed (the same samples, the same arithmetic text:
 * csrc/cemp_math.h), and no bit of it depends on the batch around it (position, neighbours, batch size, launch geometry, the LDS size of
 * the launch).
 * desc_cemp_batch_max_degree: the longest CSR row the sampler stages (4096).
 * desc_cemp_batch_create: validates every problem and refuses -- before any device work, naming the problem -- an empty edge list and a
 * node of more neighbours than desc_cemp_batch_max_degree() (DESC_ERR_INVALID: solve it with CEMP); m_total * nsample >= 2^31 is
 * DESC_ERR_TOO_LARGE.  seeds: one sampling seed per problem, or NULL (`seed` for every problem).  count == 0 is legal.  Without a device:
 * DESC_ERR_HIP and *out = NULL.
 * desc_cemp_batch_sizes: node_off[count+1], edge_off[count+1] (each nullable).
 * desc_cemp_batch_get_samples: what create sampled, for parity tests; each array nullable.  e_jk / e_ki / s0: edge_off[count] * nsample
 * entries, slot t of edge e of problem b at (edge_off[b] + e) * nsample + t; edge ids LOCAL to the problem, -1 (and s0 = 0) in the slots of
 * an edge without a 3-cycle; has_cycle: one byte per edge.
 * desc_cemp_batch_run: :107-128 with beta[min(it, n_beta - 1)] in round it, max_iter >= 0 rounds (0: the initial means of :102-103);
 * s_vec: edge_off[count] doubles in the library's edge order.  The handle may be run any number of times: every run starts from the
 * initial means. */
typedef struct desc_cemp_batch desc_cemp_batch;   /* opaque */
typedef struct desc_cemp_batch_timings {
    double ms_structure;      /* validation + per-problem CSR + degree maxima (wall clock of create's host part) */
    double ms_upload;         /* host -> HBM (create)                                                              */
    double ms_build;          /* sampling + S0 + initial means: the one launch of create, wall clock               */
    double ms_rounds;         /* the rounds and the download (desc_cemp_batch_run), wall clock                     */
    double ms_total;          /* wall clock of desc_cemp_batch_run                                                 */
} desc_cemp_batch_timings;    /* 40 bytes */
int32_t desc_cemp_batch_max_degree(void);
int desc_cemp_batch_create(const desc_problem* probs, int32_t count, int32_t nsample, uint64_t seed, const uint64_t* seeds /* nullable */,
                           int32_t device, desc_cemp_batch** out);
int desc_cemp_batch_sizes(const desc_cemp_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off);
int desc_cemp_batch_get_samples(desc_cemp_batch* h, int32_t* e_jk, int32_t* e_ki, double* s0, uint8_t* has_cycle);
int desc_cemp_batch_run(desc_cemp_batch* h, const double* beta, int32_t n_beta, int32_t max_iter, double* s_vec,
                        desc_cemp_batch_timings* timings /* nullable */);
void desc_cemp_batch_destroy(desc_cemp_batch* h);

/* The tree step of MPLS (Algorithms/MPLS.m:160-193) for B independent small problems in ONE launch: one workgroup per problem runs Prim
 * from node 1 under desc_mst_run's edge order (fl(S + 1), then the index in the (i, j)-sorted list: total, so the tree is unique and is
 * desc_mst_run's); rooting and propagation (:171-193) run per problem on host threads with desc_mst_run's own code.  Problem b's R and
 * tree edges are bit for bit what desc_mst_run gives for it.
 * desc_mst_batch_max_n: the largest problem (nodes) the tree kernel takes (4096).
 * desc_mst_batch_check: the host part alone (no device; rij is not read and may be NULL): DESC_ERR_INVALID naming the problem for an empty edge list, n >
 * desc_mst_batch_max_n() (solve it with MST / MPLS) and a disconnected graph (union-find; a node id that no edge touches is a component).
 * desc_mst_batch_run: the same checks and a non-finite s_vec entry are refused before any device work.  s_vec: the concatenated S_vec in
 * the library's edge order; R_out: problem b's 3x3xn_b column-major blocks at 9 * node_off[b] (node_off = the running sum of n);
 * tree_edges (nullable): problem b's n_b - 1 edge ids, local and ascending, at node_off[b] - b.  A step of Prim that finds no edge
 * leaving the tree is DESC_ERR_STATE naming the problem. */
typedef struct desc_mst_batch_timings {
    double ms_structure;      /* validation + connectivity + per-problem CSR (host)      */
    double ms_upload;         /* host -> HBM                                              */
    double ms_tree;           /* the tree launch and the download of its edges            */
    double ms_propagate;      /* rooting and propagation on host threads                  */
    double ms_total;          /* wall clock of desc_mst_batch_run                         */
} desc_mst_batch_timings;     /* 40 bytes */
int32_t desc_mst_batch_max_n(void);
int desc_mst_batch_check(const desc_problem* probs, int32_t count);
int desc_mst_batch_run(const desc_problem* probs, int32_t count, const double* s_vec, int32_t device, double* R_out,
                       int32_t* tree_edges /* nullable */, desc_mst_batch_timings* timings /* nullable */);

/* The DESC refinement tail (Algorithms/DESC.m:265-313, desc_refine_run) for B independent small problems in ONE launch: the last stage
 * of DESC() behind desc_pgd_batch_* and desc_gcw_batch_*.  One workgroup per problem runs the whole loop on the chip -- the edge log map,
 * the normal equations, the Jacobi-PCG with its probe every 25 steps, the node update and the score, the residuals, an exact selection
 * of the quantile's two order statistics, the new weights -- with the per-node state in LDS and no host round trip.  The arithmetic is
 * the text desc_refine_run's kernels run (csrc/laa_math.h) and every sum is taken in desc_refine_run's order: problem b's R_out and
 * record (iters, score, cg_iters, cg_unconverged, cg_residual) are bit for bit what desc_refine_run gives for it, and no bit of them
 * depends on the batch around it (position, neighbours, batch size, the LDS size of the launch).
 * desc_refine_batch_max_n: the largest n whose per-node state (26 doubles) fits the 160 KiB of LDS a workgroup may declare (748).
 * desc_refine_batch_create: validates every problem and refuses -- before any device work, naming the problem -- an empty edge list and
 * n > desc_refine_batch_max_n() (DESC_ERR_INVALID: solve it with DESC); builds the per-problem CSR (local ids) and the incidence signs
 * and uploads rotations and indices in one copy each.  count == 0 is legal and touches no device.  Without a device: DESC_ERR_HIP and
 * *out = NULL.  The handle may be run any number of times.
 * desc_refine_batch_sizes: node_off[count+1], edge_off[count+1] (each nullable).
 * desc_refine_batch_run: s_vec = the edge_off[count] concatenated S_vec in the library's edge order; R_init / R_out: problem b's 3x3xn_b
 * column-major blocks at 9 * node_off[b]; infos: count entries (ms_total = the call's; verbose is not read: the batch prints nothing,
 * not even the warning about a PCG solve that stopped at its cap -- cg_unconverged says so).  stop_threshold <= 0: 1e-3, max_iters <=
 * 0: 100, as desc_refine_run_dev.  Refused before any device work, naming the problem: a negative or non-finite s_vec entry, a
 * non-finite R_init entry (DESC_ERR_INVALID).  A problem whose selection finds no candidate or whose score is not finite is
 * DESC_ERR_STATE naming the problem.  That is the one place where the batch differs from desc_refine_run, which returns DESC_OK there
 * (it leaves its loop on a NaN score and goes on iterating on +inf): "bit for bit" above holds for every problem whose scores are finite. */
typedef struct desc_refine_batch desc_refine_batch;   /* opaque */
typedef struct desc_refine_batch_timings {
    double ms_structure;      /* validation + per-problem CSR + incidence signs (wall clock of create's host part) */
    double ms_upload;         /* host -> HBM (create)                                                                */
    double ms_input;          /* run: the checks of s_vec / R_init and their copy to HBM                             */
    double ms_refine;         /* the refinement launch, device time (HIP events)                                     */
    double ms_total;          /* wall clock of desc_refine_batch_run                                                 */
} desc_refine_batch_timings;  /* 40 bytes */
int32_t desc_refine_batch_max_n(void);
int desc_refine_batch_create(const desc_problem* probs, int32_t count, int32_t device, desc_refine_batch** out);
int desc_refine_batch_sizes(const desc_refine_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off);
int desc_refine_batch_run(desc_refine_batch* h, const double* s_vec, const double* R_init, double stop_threshold, int32_t max_iters,
                          double* R_out, desc_refine_info* infos, desc_refine_batch_timings* timings /* nullable */);
void desc_refine_batch_destroy(desc_refine_batch* h);

/* The MPLS loop (Algorithms/MPLS.m:196-254, the loop of desc_mpls_run) for B independent small problems in ONE launch, on a CEMP batch
 * handle: the last stage of MPLS() behind desc_cemp_batch_run (SVec) and desc_mst_batch_run (R_init).  The handle already owns the CSR,
 * the rotations and the sampled cycles; one workgroup per problem runs the whole loop on the chip -- the Weighted-LAA step exactly as
 * desc_refine_batch_run runs it (one text: csrc/laa_wg.h), the residuals, the H step through CEMP's samples (csrc/cemp_math.h; an edge
 * without a 3-cycle takes the reference's 2/3 rule), the convex combination, the quantile under the iteration's tau by an exact
 * selection, the new weights -- with the per-node state (26 doubles) in LDS and no host round trip.  Problem b's R_est and record are bit
 * for bit what desc_mpls_run's loop gives for it from the same s_vec and R_init, and no bit of them depends on the batch around it.
 * desc_mpls_batch_max_n: the largest problem (nodes) the loop takes: desc_refine_batch_max_n() (748).
 * desc_mpls_batch_run: s_vec = the edge_off[count] concatenated SVec in the library's edge order (what desc_cemp_batch_run returned);
 * R_init / R_est: problem b's 3x3xn_b column-major blocks at 9 * node_off[b]; beta / tau / alpha: MPLS_parameters.reweighting /
 * .thresholding / .cycle_info_ratio, each padded by repeating its last entry (MPLS.m:47-63); stop_threshold and max_iter as
 * desc_mpls_params (max_iter <= 1: no iteration, R_est = q2R(R2Q(R_init))).  infos: count entries with desc_mpls_info's meaning (m_pos =
 * the problem's edges with a 3-cycle; ms_loop / ms_total = the call's, ms_cemp = ms_mst = 0).  At its first call the handle allocates the
 * loop's arrays and uploads the incidence signs (ms_setup; 0 afterwards).  The handle may be run any number of times, and
 * desc_cemp_batch_run and desc_mpls_batch_run may alternate on it.  The call prints nothing.  Refused before any device work
 * (DESC_ERR_INVALID), naming the problem: NULL arguments; n_beta, n_tau or n_alpha < 1; a problem of more than desc_mpls_batch_max_n()
 * nodes (solve it with MPLS); a negative or non-finite s_vec entry; a non-finite R_init entry.  An empty batch returns DESC_OK.  A
 * problem whose selection finds no candidate or whose score is not finite is DESC_ERR_STATE naming the problem and the step (there
 * desc_mpls_run returns DESC_OK, leaving its loop on a NaN score: "bit for bit" holds for every problem whose scores are finite). */
typedef struct desc_mpls_batch_timings {
    double ms_setup;          /* first call: the loop's arrays, the incidence signs, the cycle counts; 0 afterwards */
    double ms_input;          /* the checks of s_vec / R_init and their copy to HBM                                */
    double ms_loop;           /* the loop's launch, device time (HIP events)                                       */
    double ms_download;       /* R_est and the records back to the host                                            */
    double ms_total;          /* wall clock of desc_mpls_batch_run                                                 */
} desc_mpls_batch_timings;    /* 40 bytes */
int32_t desc_mpls_batch_max_n(void);
int desc_mpls_batch_run(desc_cemp_batch* h, const double* s_vec, const double* R_init, double stop_threshold, int32_t max_iter,
                        const double* beta, int32_t n_beta, const double* tau, int32_t n_tau, const double* alpha, int32_t n_alpha,
                        double* R_est, desc_mpls_info* infos, desc_mpls_batch_timings* timings /* nullable */);

/* IRLS_GM / IRLS_L12 (desc_irls_run) for B independent small, connected problems in TWO launches (csrc/irls_batch.hip): the last two rows
 * of Demo/compare_algorithms.m for a Monte-Carlo batch.  Launch A checks and projects the edges of all problems (IRLS_GM.m:82-93) and
 * leaves per problem the smallest failing caller row and a warning count; launch B runs one workgroup per problem through stages 4 and
 * 5 of desc_irls_run_dev -- the spanning-tree start, the L1 loop with its primal-dual steps, their Newton systems by the PCG with
 * per-coordinate weights and breakdown tracking, Q = R2Q(R_l1), the reweighted loop -- with the per-node state (34 doubles) in LDS and
 * no host round trip.  The per-element arithmetic and the scalar rules are one text with the single call (csrc/irls_math.h,
 * csrc/laa_math.h, csrc/laa_wg.h) and every sum is taken in the single call's order (the 256 virtual blocks of its partial-reduction
 * kernels included): problem b's R_out, R_l1 and record (every field of desc_irls_info but the ms_*) are bit for bit what desc_irls_run
 * gives for it with the same order, and no bit of them depends on the batch around it.
 * desc_irls_batch_max_n: the largest n whose per-node state fits the 160 KiB of LDS a workgroup may declare next to the kernel's fixed
 * LDS (557; at least the eigen-solve's 278).
 * desc_irls_batch_create: orders (nullable, and each entry nullable) = per problem desc_irls_params.order, the caller's 0-based row of
 * every edge: the row order of the spanning-tree start and of the error message.  Validates every problem and refuses -- before any
 * device work, naming the problem -- an empty edge list, an order that is no permutation, n > desc_irls_batch_max_n() and a graph that
 * is not connected (DESC_ERR_INVALID: solve it with IRLS_GM / IRLS_L12; component extraction stays with the single call).  Builds the
 * per-problem CSR, the incidence signs and the tree sequences (the graph part of BoxMedianSO3Graph.m:79-114, in the caller's row
 * order) on the host, checks the kernel's fixed LDS (hipFuncGetAttributes) plus the launch's dynamic LDS against 160 KiB, uploads.
 * count == 0 is legal and touches no device.  Without a device: DESC_ERR_HIP and *out = NULL.  The handle may be run any number of
 * times, in either mode.
 * desc_irls_batch_sizes: node_off[count+1], edge_off[count+1] (each nullable).
 * desc_irls_batch_run: mode DESC_IRLS_GM / DESC_IRLS_L12; sigma_deg, max_iter_l1, max_iter_irls as desc_irls_params (<= 0: 5, 10, 100),
 * one set for the whole batch; there is no R_init.  R_out / R_l1 (nullable): problem b's 3x3xn_b column-major blocks at 9 * node_off[b];
 * infos: count entries (comp_nodes / comp_edges = the problem's n and m; ms_total = the call's, the other ms_* 0: the stage times are
 * the batch's, in timings).  The call prints nothing: warned_edges and cg_unconverged say what the single call warns about.  An edge
 * block with det <= 0 or with all three singular values off 1 by >= 0.1 is DESC_ERR_INVALID naming the problem and the 1-based caller
 * row with the single call's numbers -- the lowest problem first, the smallest caller row within it. */
typedef struct desc_irls_batch desc_irls_batch;   /* opaque */
typedef struct desc_irls_batch_timings {
    double ms_structure;      /* validation + per-problem CSR + incidence signs + tree sequences (create's host part) */
    double ms_upload;         /* host -> HBM (create)                                                                */
    double ms_project;        /* run: launch A and the read-back of its flags (wall clock)                            */
    double ms_solve;          /* launch B, device time (HIP events)                                                  */
    double ms_total;          /* wall clock of desc_irls_batch_run                                                   */
} desc_irls_batch_timings;    /* 40 bytes */
int32_t desc_irls_batch_max_n(void);
int desc_irls_batch_create(const desc_problem* probs, int32_t count, const int32_t* const* orders /* nullable */, int32_t device,
                           desc_irls_batch** out);
int desc_irls_batch_sizes(const desc_irls_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off);
int desc_irls_batch_run(desc_irls_batch* h, int32_t mode, double sigma_deg, int32_t max_iter_l1, int32_t max_iter_irls, double* R_out,
                        double* R_l1 /* nullable */, desc_irls_info* infos, desc_irls_batch_timings* timings /* nullable */);
void desc_irls_batch_destroy(desc_irls_batch* h);
/* The host half of the spanning-tree start alone (no device; tests and the batched call's refusals): the passes of
 * BoxMedianSO3Graph.m:79-114 over the edges in the caller's row order (order nullable: the edge order) from node 1.  seq (nullable,
 * n - 1 entries): one entry 2 e + dir per reached node in the order the reference sets them (dir 0: Q(j) from Q(i) of edge e, dir 1:
 * Q(i) from Q(j)); *reached: the nodes reached, n exactly when the graph is connected. */
int desc_irls_tree_sequence(const desc_problem* prob, const int32_t* order, int32_t* seq, int64_t* reached);

/* The LP of linprog_sij (desc_lp_sij_run_dev's samples, incidence and PDHG loop) for B independent small problems at once: the variables
 * and cycles of all problems lie behind one another and every launch of the loop -- two per step, about ten per check -- is shared by the
 * batch (csrc/lp_batch.hip; the arithmetic and the decision rule are csrc/lp_math.h, one text with the single call).  Problem b's s_vec,
 * y, k and record are bit for bit what desc_lp_sij_run_dev returns for it alone with the same seed, nsample and parameters, and no bit of
 * them depends on the batch around it: every sum of a problem runs over that problem's own virtual grid (the grid the single call
 * launches for it), and after a check one kernel takes each problem's decisions (restart, stop, returned point) on the device from the
 * records the host reads in the single call.  The host reads one int32 per check: the number of problems still running.  A problem that
 * stopped is frozen while the others run on; its iters is the step of its stop.
 * desc_lp_batch_plan: the host half of create without a device, for sizing and tests: per problem nsample, m_pos, the offsets of its
 * variables and of its cycles (count + 1 entries each) and the blocks of its two virtual grids; every array nullable.
 * desc_lp_batch_create: everything that does not depend on tol, max_iter, check_every or restart.  nsample (nullable): count entries, 0 =
 * the rule of linprog_sij.m:43 evaluated for that problem alone (NULL: the rule for all); seeds (nullable: 0 for all): count sampling
 * keys.  Variable l of problem b is the batch's variable var_off[b] + l, cycle t of it the batch's cycle row_off[b] + l * nsample_b + t.
 * Refused before any device work, naming the problem: what desc_problem validation refuses, an empty edge list, nsample < 0
 * (DESC_ERR_INVALID); a node of more neighbours than desc_cemp_batch_max_degree() = 4096, the cap of the batched sampler, shared with
 * desc_cemp_batch_create (DESC_ERR_INVALID: solve it with linprog_sij); a batch whose LP rows 2 * sum(m_pos_b * nsample_b) reach 2^31
 * (DESC_ERR_TOO_LARGE: split the batch).  A problem without a triangle is the empty LP: s_vec = 1, iters = 0, converged = 1.
 * desc_lp_batch_sizes: node_off / edge_off / var_off / row_off: count + 1 entries; nsample / m_pos: count entries; each nullable.
 * desc_lp_batch_get_samples: pos_edges: var_off[count] 0-based edge ids (sorted order, local to the problem), the LP's variables; k:
 * row_off[count] sampled third nodes, 1-based; what params->pos_out and k_out of the single call receive.  Each nullable.
 * desc_lp_batch_run: params (NULL: the defaults): tol, max_iter, check_every and restart are read, nsample and seed belong to create,
 * verbose is ignored (the call prints nothing).  s_vec: edge_off[count] doubles; y (nullable): 2 row_off[count] doubles, each problem's
 * duals of its returned point; infos: count records (ms_loop = ms_total = the call's; the other stage times are 0).  max_iter = 0 returns
 * the start x = 0, y = 0 and its record.  Problems that stop at max_iter with tol > 0 are named in one warning line on stderr.  The handle
 * may be run any number of times with other parameters; two handles may be alive at once.  An empty batch returns DESC_OK. */
typedef struct desc_lp_batch desc_lp_batch;   /* opaque */
typedef struct desc_lp_batch_timings {
    double ms_structure;      /* host: validation, CSR, codegrees, nsample, offsets, workgroup tables (create)      */
    double ms_upload;         /* host -> device copies and allocations (create)                                    */
    double ms_build;          /* samples, S0Mat and the transposed incidence (create), wall clock                  */
    double ms_loop;           /* the loop and the downloads (desc_lp_batch_run), wall clock                        */
    double ms_total;          /* wall clock of desc_lp_batch_run                                                   */
} desc_lp_batch_timings;      /* 40 bytes */
int desc_lp_batch_plan(const desc_problem* probs, int32_t count, const int32_t* nsample /* nullable */, int32_t* nsample_out, int64_t* m_pos,
                       int64_t* var_off, int64_t* row_off, int32_t* ncol, int32_t* nrow);
int desc_lp_batch_create(const desc_problem* probs, int32_t count, const int32_t* nsample /* nullable */, const uint64_t* seeds /* nullable */,
                         int32_t device, desc_lp_batch** out);
int desc_lp_batch_sizes(const desc_lp_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off, int32_t* nsample, int64_t* m_pos,
                        int64_t* var_off, int64_t* row_off);
int desc_lp_batch_get_samples(desc_lp_batch* h, int32_t* pos_edges, int32_t* k);
int desc_lp_batch_run(desc_lp_batch* h, const desc_lp_params* params, double* s_vec, double* y /* nullable */, desc_lp_info* infos,
                      desc_lp_batch_timings* timings /* nullable */);
void desc_lp_batch_destroy(desc_lp_batch* h);

/* ------------------------------------------------- batched problem generator -- */
/* Models/Uniform_Topology.m:24-101 and Models/Nonuniform_Topology.m:26-147 for B problems in one GPU pass (csrc/models_batch.hip): what
 * a Monte-Carlo study draws in front of the *_batch solvers.  MATLAB's RNG streams cannot be matched; this is a seeded restatement of
 * the same distributions -- a third one, next to MATLAB's and to desc_amd/models.py's NumPy streams, whose draws it does NOT reproduce
 * for the same seed.  tests/models_batch_oracle.py restates the definition below in NumPy.
 *
 * Keys.  Every random number of problem b is a pure function of (seed_b, stream, sub, id, c):
 *     desc_models_key(seed, stream, sub, id, c) = desc_sample_key(desc_sample_key(seed, stream, sub), id, c)
 * with ids counted inside the problem (0-based node v, 0-based edge e in the (i, j)-sorted list, pair index t = i n - i (i + 1) / 2 +
 * (j - i - 1) of the 0-based pair i < j), so that no bit of a problem depends on the batch around it.
 *   uniform draw   u = (key >> 11) * 2^-53, an exact double in [0, 1)
 *   normal draw c  z = sqrt(-2 log(u1)) * cos(6.283185307179586 * u2) with u1 = ((key(.., 2c) >> 12) + 0.5) * 2^-52 in (0, 1) and
 *                  u2 = (key(.., 2c + 1) >> 11) * 2^-53
 *   normal block   nine normals c = 0..8; c is entry (c mod 3, c div 3): the block's column-major memory order, as randn(3) fills it
 *   projection     P(Q) = U diag(1, 1, det(U V')) V' of Q = U S V' (Uniform_Topology.m:41-44, :61-65); a Haar rotation is P(normal block)
 * Streams (sub = 0 unless stated):
 *   DESC_MODELS_STREAM_EDGE    id = t, c = 0: the pair is an edge iff u < p                       (Uniform_Topology.m:29)
 *   DESC_MODELS_STREAM_RORIG   id = v: the normal block of R_orig(:,:,v)                          (:40-45)
 *   DESC_MODELS_STREAM_RCORR   id = v: the normal block of R_corr / R_crpt(:,:,v)                 (:69-74; Nonuniform_Topology.m:66-71)
 *   DESC_MODELS_STREAM_CORRUPT id = e, c = 0: a noise edge iff u >= q, else corrupted             (Uniform_Topology.m:53)
 *   DESC_MODELS_STREAM_NOISE   id = e: the normal block N_e of the additive noise                 (:58-59, :86; Nonuniform_Topology.m:121-127)
 *   DESC_MODELS_STREAM_HAAR    id = e: the normal block of a 'uniform' corrupted edge             (Uniform_Topology.m:77-82)
 *   DESC_MODELS_STREAM_NODE    id = v, c = 0: the node key.  The node order is ascending (key, v); the corrupted nodes are the first
 *                              floor(n * p_node_crpt) of it                                       (Nonuniform_Topology.m:60-62)
 *   DESC_MODELS_STREAM_SELECT  sub = v, id = e, c = 0: node v corrupts the floor(p_edge_crpt * deg_v) incident edges with the smallest
 *                              (key, e)                                                           (:77-82)
 *   DESC_MODELS_STREAM_R0      sub = w, id = e: the normal block of R0 drawn by the winning node w for edge e   (:88-91)
 * Uniform (mode DESC_MODELS_UNIFORM, any other value: self-consistent, as :76,83): a noise edge gets P(Rij_orig + sigma N_e); a
 * corrupted edge P(Haar block) or, self-consistent, P(R_corr_i R_corr_j' + sigma N_e).
 * Nonuniform (modes UNIFORM | SELF_CONSISTENT | ADV): an edge selected by both endpoints belongs to the endpoint later in the node
 * order (the later iteration of :76 overwrites).  With w the winner and x the other endpoint, M = R0 | R_crpt_w R_crpt_x' | R_crpt_w
 * R_orig_x'; the edge's block becomes M if w is the edge's first node (IndMat > 0, :86) and M' otherwise; an edge nobody selected keeps
 * Rij_orig.  Then every edge gets P(block + s N_e), s = sigma_out on a corrupted edge and sigma_in elsewhere (:121-137).
 * ErrVec = |acos((trace(Rij_orig' RijMat) - 1) / 2)| / pi with the extended |acos| of the cycle kernels for an argument a rounding error
 * outside [-1, 1].  Operand order on the device: Rij_orig(r, c) = sum_k Ri(r, k) Rj(c, k) in ascending k from 0.0; Q = block + s * N.
 *
 * desc_models_batch_max_n: the largest n (65536): n (n - 1) / 2 edges stay below 2^31.
 * desc_models_batch_create: validates on the host and refuses -- before the device is touched, naming the problem -- n < 2 or above the
 * cap, a probability (p, q, p_node_crpt, p_edge_crpt) outside [0, 1] or not finite, a negative or non-finite sigma, an unknown kind, an
 * unknown mode of a Nonuniform problem (DESC_ERR_INVALID); a batch of 2^31 nodes or more or whose expected edge count sum(p_b n_b (n_b -
 * 1) / 2) reaches 2^30 (DESC_ERR_TOO_LARGE).  Then the graph pass runs: one wave per (problem, row) counts the row's edges (ballot +
 * popcount), a scan per problem gives the row offsets, the host reads the count edge totals, and a second pass writes the sorted edge
 * list.  No n x n array exists.  A problem that draws no edge is legal (m = 0).  count == 0 is legal and touches no device.  Without a
 * device: DESC_ERR_HIP and *out = NULL.
 * desc_models_batch_sizes: m_per_problem[count].
 * desc_models_batch_fetch: the node, selection and edge passes, and the copy of the concatenated arrays (problem after problem) into
 * the caller's buffers, each nullable: ind_i / ind_j (M, 0-based, as desc_problem), rij / rij_orig (M x 9, column-major blocks),
 * r_orig (N x 9), err_vec (M), corrupted (M).  May be called again; the result is the same. */
#define DESC_MODELS_KIND_UNIFORM      0
#define DESC_MODELS_KIND_NONUNIFORM   1
#define DESC_MODELS_UNIFORM           0
#define DESC_MODELS_SELF_CONSISTENT   1
#define DESC_MODELS_ADV               2
enum { DESC_MODELS_STREAM_EDGE = 1, DESC_MODELS_STREAM_RORIG, DESC_MODELS_STREAM_RCORR, DESC_MODELS_STREAM_CORRUPT,
       DESC_MODELS_STREAM_NOISE, DESC_MODELS_STREAM_HAAR, DESC_MODELS_STREAM_NODE, DESC_MODELS_STREAM_SELECT, DESC_MODELS_STREAM_R0 };
typedef struct desc_model_spec {
    int32_t kind;             /* DESC_MODELS_KIND_*                                                           */
    int32_t n;
    double p;                 /* edge probability                                                             */
    double q;                 /* Uniform: corruption probability                                              */
    double p_node_crpt;       /* Nonuniform                                                                   */
    double p_edge_crpt;       /* Nonuniform                                                                   */
    double sigma;             /* Uniform                                                                      */
    double sigma_in;          /* Nonuniform: noise of the edges nobody corrupted                              */
    double sigma_out;         /* Nonuniform: noise of the corrupted edges                                     */
    int32_t mode;             /* DESC_MODELS_UNIFORM | _SELF_CONSISTENT | _ADV (Nonuniform only)              */
    int32_t reserved;
    uint64_t seed;
} desc_model_spec;            /* 80 bytes */
typedef struct desc_models_batch desc_models_batch;   /* opaque */
typedef struct desc_models_batch_timings {
    double ms_graph;          /* validation, upload and the graph pass (create), wall clock                   */
    double ms_nodes;          /* the node pass and, with a Nonuniform problem, marking and selection          */
    double ms_edges;          /* the edge pass                                                                */
    double ms_copy;           /* device -> host copies into the caller's buffers                              */
    double ms_total;          /* ms_graph + wall clock of desc_models_batch_fetch                             */
} desc_models_batch_timings;  /* 40 bytes */
uint64_t desc_models_key(uint64_t seed, uint64_t stream, uint64_t sub, uint64_t id, uint64_t c);
int32_t desc_models_batch_max_n(void);
int desc_models_batch_create(const desc_model_spec* specs, int32_t count, int32_t device, desc_models_batch** out);
int desc_models_batch_sizes(const desc_models_batch* h, int64_t* m_per_problem);
int desc_models_batch_fetch(desc_models_batch* h, int32_t* ind_i, int32_t* ind_j, double* rij, double* rij_orig, double* r_orig,
                            double* err_vec, uint8_t* corrupted, desc_models_batch_timings* timings /* nullable */);
void desc_models_batch_destroy(desc_models_batch* h);
/* Test hooks (tests/test_gpu_models_batch.py): the device's draws for ids id0 .. id0 + count - 1 of (seed, stream, sub): the uniform
 * draw of component c, and the normal draw c.  out: count doubles.  NULL out or a negative count: DESC_ERR_INVALID. */
int desc_test_models_uniform(uint64_t seed, uint64_t stream, uint64_t sub, uint64_t id0, int64_t count, uint64_t c, int32_t device, double* out);
int desc_test_models_normal(uint64_t seed, uint64_t stream, uint64_t sub, uint64_t id0, int64_t count, uint64_t c, int32_t device, double* out);

/* ------------------------------------------------- batched rotation alignment -- */
/* Utils/Rotation_Alignment.m:13-38 for B problems in one GPU pass (csrc/align_batch.hip): the scoring behind the *_batch solvers of a
 * Monte-Carlo study.  One launch, one workgroup of 256 threads per problem.  The problems' 3 x 3 x n_b column-major blocks lie behind
 * one another, problem b's from 9 * node_off[b] (as R_out of desc_gcw_batch_run); N = sum(n).  tests/align_batch_oracle.py restates
 * the orders below in NumPy.
 *
 * Operand orders on the device (the library is built without contraction; they are part of the interface):
 *   A (:18-22)        thread t of the workgroup takes the nodes t, t + 256, ... in ascending order; per node the entry (r, c) is
 *                     sum_a R_est(a, r) R_gt(a, c) in ascending a from 0.0, added to the thread's running sum of that entry.  The 256
 *                     partials: the 64 lanes of a wave by the fixed butterfly desc_selftest_group_sum exposes (G = 64), then
 *                     ((wave 0 + wave 1) + wave 2) + wave 3.
 *   R_align (:24-25)  U1 diag(1, 1, det(U1 V1')) V1' of A by a one-sided Jacobi SVD (A V = U S; pairs (0,1), (0,2), (1,2), at most 40
 *                     sweeps, a pair is skipped when |g| <= 1e-17 sqrt(a b)), the singular values sorted descending; u1 = a1 / |a1|,
 *                     u2 = (a2 - (u1'a2) u1) normalised, the third left vector det(V) (u1 x u2):
 *                     R_align(r, c) = (u1(r) v1(c) + u2(r) v2(c)) + u3(r) v3(c).  Ill-defined as (s2 + sign(det A) s3) / s1 -> 0.
 *   R_out (:30-32)    R_out_k(r, c) = sum_j R_est_k(r, j) R_align(j, c) in ascending j from 0.0.
 *   err (:33-34)      tr = sum of R_gt_k .* R_out_k over the nine entries in column-major order from 0.0;
 *                     err_k = |acos((tr - 1) / 2)| / pi * 180 (degrees), with the extended |acos| of the cycle kernels for an
 *                     argument a rounding error outside [-1, 1].
 *   mean_error (:35)  thread t adds err_t, err_(t + 256), ... from 0.0; the 256 partials as for A; the total / n.
 *   median_error (:36) MATLAB's median by an exact selection: n odd, the order statistic of rank (n + 1) / 2; n even, a + (b - a) / 2
 *                     of the two middle order statistics a <= b.
 * No bit of a problem depends on the batch around it or on its position.
 *
 * desc_align_batch_create: n[count], R_gt: 9 N doubles.  Validates on the host and refuses -- before the device is touched, naming the
 * problem -- n_b < 1, a non-finite entry of R_gt (naming the 1-based node as well) (DESC_ERR_INVALID); 9 N >= 2^31, i.e. 2^31 / 9 nodes
 * or more (DESC_ERR_TOO_LARGE, before R_gt is read).  The handle keeps the ground truth on the device.  count == 0 is legal and touches no
 * device.  Without a device: DESC_ERR_HIP and *out = NULL.
 * desc_align_batch_sizes: *count and node_off[count + 1], each nullable.
 * desc_align_batch_run: scores R_est (9 N) against the handle's ground truth; may be called any number of times.  A non-finite entry of
 * R_est is refused as in create, before this call touches the device.  R_out (9 N) and err (N) are nullable -- R_out is three quarters
 * of the bytes that come back --; R_align (9 count), mean_error and median_error (count) are required. */
typedef struct desc_align_batch desc_align_batch;   /* opaque */
typedef struct desc_align_batch_timings {
    double ms_upload;         /* the finite check of R_est and its upload, wall clock                        */
    double ms_align;          /* the launch, wall clock to the drained stream                                 */
    double ms_copy;           /* device -> host copies into the caller's buffers                              */
    double ms_total;          /* wall clock of desc_align_batch_run                                           */
} desc_align_batch_timings;   /* 32 bytes */
int desc_align_batch_create(const int32_t* n, const double* R_gt, int32_t count, int32_t device, desc_align_batch** out);
int desc_align_batch_sizes(const desc_align_batch* h, int32_t* count, int64_t* node_off);
int desc_align_batch_run(desc_align_batch* h, const double* R_est, double* R_out /* nullable */, double* R_align, double* err /* nullable */,
                         double* mean_error, double* median_error, desc_align_batch_timings* timings /* nullable */);
void desc_align_batch_destroy(desc_align_batch* h);
/* Test hook (tests/test_gpu_align_batch.py): the projection of R_align alone on count column-major blocks A (destroyed on the device
 * only), one thread per block.  NULL A or R, or a negative count: DESC_ERR_INVALID. */
int desc_test_align_project(const double* A, int64_t count, int32_t device, double* R);

/* A problem set resident on the device across calls: the problems of B independent instances validated, laid out and uploaded ONCE, for
 * every batched handle created on it.  On the device: ii, jj (local 0-based endpoints, M entries), rowptr (problem b's n_b + 1 entries
 * at node_off[b] + b), adj and adj_eid (problem b's 2 m_b entries at 2 edge_off[b], local ids), rij (9 M doubles, column-major blocks)
 * -- the layout the batched handles make for themselves.  On the host: the sizes, the offsets, ii and jj; the CSR only where the host
 * builder made it.  After create the arrays are read-only.
 * desc_problem_batch_create: refuses what desc_gcw_batch_create refuses of a problem, in its words and order ("problem b: ...", an empty
 * edge list, 2^30 edges in total), before any device work.  csr_where = DESC_BUILD_HOST builds the CSR on host threads and uploads it;
 * DESC_BUILD_DEVICE uploads ii and jj and builds the same CSR, element for element, in one launch (one workgroup per problem, integer
 * arithmetic only, no atomics; it has no size cap).  count == 0 is legal and touches no device.
 * desc_problem_batch_from_models: the set of a generator handle without a host copy of any rotation.  Runs the generator's node and
 * edge passes if no fetch has; copies ii, jj and rij device to device (the models handle may be destroyed first); n_b = the largest
 * endpoint + 1 (what marshalling the fetched list gives, not the spec's n); a problem that drew no edge is refused (DESC_ERR_INVALID,
 * "problem b: empty edge list"); the CSR is built on the device.  Device-to-host traffic: ii and jj (8 bytes per edge).
 * desc_problem_batch_fetch: each argument nullable; ii / jj from the host mirror, rij and a device-built CSR come down.
 * desc_problem_batch_built_where: the builder of the set's CSR.  desc_problem_batch_bytes: what the set copied up and down so far.
 * desc_problem_batch_destroy drops the caller's reference: handles created on the set keep it alive, the memory goes with the last owner.
 *
 * desc_gcw_batch_create_on / desc_refine_batch_create_on / desc_pgd_batch_create_on: the handle of desc_*_batch_create(_where) on the
 * set's device, borrowing the set's device arrays.  Each refuses what its create refuses (the caps, eig, where: same words, before any
 * device work); what create derives from the CSR is formed on the device (the refinement's sign per slot, the device builder's edge ->
 * problem map), so the uploads of a create_on are O(B) bytes.  desc_pgd_batch_create_on takes either builder (the host builder reads
 * the set's host ii / jj; p->device is not read); the device builder's silent fallback is unchanged.  The run functions are unchanged
 * and give the bits of a handle created from the host arrays.  desc_*_batch_bytes: the bytes a handle's create copied up / down;
 * a handle created from a problem list (desc_{gcw,refine,cemp,irls}_batch_create) counts what the set it made for itself copied, too.
 *
 * desc_cemp_batch_create_on / desc_irls_batch_create_on: the same for the CEMP handle (with desc_mpls_batch_run on it) and the IRLS
 * handle.  The degree cap of the sampler is checked on the set's host row starts or, for a device-built CSR, on a count over its host
 * endpoints; the IRLS cap, the order check and the connectivity refusal run on the set's host endpoints.  Uploads: the CEMP problem
 * records (32 bytes per problem); the IRLS tree sequences (4 bytes per node) and, only where some problem's order is not the identity,
 * the row orders (4 bytes per edge).  The edge -> problem maps, the signs per slot and identity orders are formed by launches.
 * desc_mst_batch_run_on: desc_mst_batch_run on the set's device: its refusals on the set's host endpoints, s_vec up (8 bytes per edge),
 * the tree kernel on the set's CSR, the 3 x 3 blocks of the n_b - 1 tree edges gathered by a launch and brought down (72 bytes per tree
 * edge) for the host's rooting and propagation.  bytes (nullable): {host -> device, device -> host} of this call. */
typedef struct desc_problem_batch desc_problem_batch;   /* opaque */
int desc_problem_batch_create(const desc_problem* probs, int32_t count, int32_t device, int32_t csr_where /* DESC_BUILD_HOST | DESC_BUILD_DEVICE */,
                              desc_problem_batch** out);
int desc_problem_batch_from_models(desc_models_batch* m, desc_problem_batch** out);
int desc_problem_batch_sizes(const desc_problem_batch* h, int32_t* count, int64_t* node_off, int64_t* edge_off);
int desc_problem_batch_fetch(desc_problem_batch* h, int32_t* ind_i, int32_t* ind_j, double* rij, int32_t* rowptr, int32_t* adj, int32_t* adj_eid);
int32_t desc_problem_batch_built_where(const desc_problem_batch* h);
int desc_problem_batch_bytes(const desc_problem_batch* h, int64_t* h2d, int64_t* d2h);
void desc_problem_batch_destroy(desc_problem_batch* h);
int desc_gcw_batch_create_on(desc_problem_batch* set, int32_t eig, desc_gcw_batch** out);
int desc_refine_batch_create_on(desc_problem_batch* set, desc_refine_batch** out);
int desc_pgd_batch_create_on(desc_problem_batch* set, const desc_params* p, const uint64_t* seeds /* count, nullable */, int32_t where,
                             desc_pgd_batch** out);
int desc_gcw_batch_bytes(const desc_gcw_batch* h, int64_t* h2d, int64_t* d2h);
int desc_refine_batch_bytes(const desc_refine_batch* h, int64_t* h2d, int64_t* d2h);
int desc_pgd_batch_bytes(const desc_pgd_batch* h, int64_t* h2d, int64_t* d2h);
int desc_cemp_batch_create_on(desc_problem_batch* set, int32_t nsample, uint64_t seed, const uint64_t* seeds /* count, nullable */,
                              desc_cemp_batch** out);
int desc_irls_batch_create_on(desc_problem_batch* set, const int32_t* const* orders /* nullable, entries nullable */, desc_irls_batch** out);
int desc_mst_batch_run_on(desc_problem_batch* set, const double* s_vec, double* R_out, int32_t* tree_edges /* nullable */,
                          desc_mst_batch_timings* timings /* nullable */, int64_t* bytes /* nullable: {h2d, d2h} of this call */);
int desc_cemp_batch_bytes(const desc_cemp_batch* h, int64_t* h2d, int64_t* d2h);
int desc_irls_batch_bytes(const desc_irls_batch* h, int64_t* h2d, int64_t* d2h);

/* One-shot: what the MEX shim calls.  Builds the structure (p->build_where),
 * uploads, runs, downloads, frees. */
int desc_pgd_solve(const desc_problem* prob, const desc_params* p, desc_result* r);

/* Host-side marshalling of the reference's argument formats (no device code; a binding that already holds 0-based int32 endpoints and
 * MATLAB's own 3 x 3 x m memory -- the MEX shim -- needs neither).
 * desc_marshal_edges: `Ind` as the caller of DESC_PGD.m:14 holds it -- m x 2 node ids, 1-based, Ind(:,1) < Ind(:,2), as doubles (MATLAB),
 * int64 or int32 -- read through element strides (row_stride, col_stride: MATLAB's column-major m x 2 = (1, m), NumPy's row-major = (2, 1))
 * into the ABI's 0-based int32 endpoints in ONE threaded pass.  *n_out = max(Ind(:)) (DESC_PGD.m:21); *sorted_out = 1 if the rows are
 * strictly ascending by (i, j) (what DESC_PGD.m:5 requires and desc_problem expects), 0 if the caller still has to sort (and to look for
 * duplicates).  DESC_ERR_INVALID: a value that is not an integer, an id < 1, or a row with Ind(:,1) >= Ind(:,2) (first offending row in the text).
 * desc_marshal_rij: out[9 l + r + 3 c] = R[r stride_r + c stride_c + perm[l] stride_l] -- any strided 3 x 3 x m array of doubles (NumPy's
 * C order: strides (3m, m, 1); MATLAB's order (1, 3, 9) is the ABI's own and needs no call) into desc_problem.rij, edges permuted by
 * `perm` (sorted position -> caller's row; NULL: identity). */
#define DESC_DTYPE_F64 0
#define DESC_DTYPE_I64 1
#define DESC_DTYPE_I32 2
int desc_marshal_edges(const void* ind, int32_t dtype, int64_t m, int64_t row_stride, int64_t col_stride,
                       int32_t* ind_i, int32_t* ind_j, int64_t* n_out, int32_t* sorted_out);
int desc_marshal_rij(const double* R, int64_t m, int64_t stride_r, int64_t stride_c, int64_t stride_l, const int64_t* perm, double* out);

/* The library parks the device blocks of destroyed handles / structures / problems for reuse by the next call (up to
 * DESC_CACHE_MB megabytes per process, default 8192: hipFree + hipMalloc of the gigabyte-sized per-cycle arrays cost 10-20 ms
 * per solve), and likewise the large host-side index vectors of its setup (up to DESC_HOST_CACHE_MB, default 1024: first-touch
 * page faults and munmap of ~200 MB cost 40 ms per solve at n = 5000).  desc_trim_memory returns everything parked to the
 * driver / the C++ runtime; result: device bytes released. */
int64_t desc_trim_memory(void);

/* Binding utilities: synchronous copies between host memory and device memory of the library's own HIP runtime
 * (a binding that implements the collectives itself, e.g. staged through host memory, must not load a second
 * runtime), after draining every stream of `device`. */
int desc_device_synchronize(int32_t device);
int desc_memcpy_d2h(void* host_dst, const void* dev_src, size_t bytes);
int desc_memcpy_h2d(void* dev_dst, const void* host_src, size_t bytes);

/* Test hook, host only (runs without a GPU): plans the band sweep of `rank` of `world` for `grid` workgroups and checks the plan's
 * invariants.  stats: 8 values out (bands, pieces, largest band's row entries, max / min cycles per workgroup, j-block-major?,
 * first / end segment of the rank). */
int desc_debug_band_plan(const desc_problem* prob, const desc_structure* s, int32_t world, int32_t rank, int32_t grid, int64_t* stats);

/* Diagnostics hook (tools/wg_clock.py): {start, end} (constant 100 MHz clock) of every workgroup of the last band sweep of a handle created
 * with DESC_DEBUG_WGCLOCK=1; returns how many workgroups were written to out[2 * cap] (0: not recorded).  When all G workgroups fit and
 * 2 * cap >= 3 * G, out[2 * G + w] = shader-clock cycles workgroup w ran for (cycles / duration = the clock frequency of the launch). */
int desc_debug_wg_clock(desc_pgd* h, uint64_t* out, int32_t cap);
/* ... and what the piece scheduler gave each of them: out[4 * w + {0,1,2,3}] = cycles, segments, pieces, CSR entries of the band rows loaded. */
int desc_debug_wg_plan(desc_pgd* h, int64_t* out, int32_t cap);

/* Test hooks (tests/test_gpu_sharded.py).  desc_debug_last_sweep: name and template arguments of the sweep kernel the handle launched last
 * ("k_sweep_band<16,4,0,512,XT>": the sharded instance), "" before the first sweep.  desc_debug_shard_layout: the exchange layout of a
 * (possibly sharded) handle -- xpos / spos: 2m entries each (CSR slot -> place of its mirror sum, DESC_PGD.m:189-190, in the reduce-scatter
 * send buffer / place of its edge's S in the gathered slices); xt: {ta, tb} per owned segment (device order), slot_ab: the CSR slots of
 * the same segments' edges; both 2 * (seg_hi - seg_lo) entries. */
const char* desc_debug_last_sweep(const desc_pgd* h);
int desc_debug_shard_layout(desc_pgd* h, int32_t* xpos, int32_t* spos, int32_t* xt, int32_t* slot_ab);

/* Measurement hook (tools/next_rows_bench.py; SURVEY.md 8d "document the MFMA measurement rather than assume"): the 3x3-block SpMM of the
 * connection matrix (Spectral.m:27-37) with unit weights, `reps` products in its vector-FMA form and in a v_mfma_f64_4x4x4 form on the
 * same operand.  out[4]: ms per product (vector FMA), ms per product (MFMA; -1: operand layout not identified), max |difference|, layout code. */
int desc_debug_spmm_variants(const desc_device_problem* dp, int32_t reps, double* out);

/* Test hook: sums `in` over aligned groups of G = 16/32/64 lanes with the kernels'
 * DPP / permlane-swap reduction; every element of a group receives the group total. */
int desc_selftest_group_sum(const double* in, double* out, int32_t count, int32_t G, int32_t device);

/* Test hooks (tests/test_gpu_laa_maps.py): one operation of the Lie-algebraic averaging core (laa.hip, irls.hip) on caller arrays
 * in host memory, launched with the kernel and the grid rule the library itself uses; nothing in the library calls them.  Quaternions
 * are 4 doubles (a, x, y, z), blocks 9 doubles column-major, per-edge / per-node vectors 3 doubles.  A NULL pointer, a negative count,
 * p outside [0, 1] or an m that differs from the device problem's returns DESC_ERR_INVALID before any device work.
 *   r2q          count blocks -> count quaternions (R2Q.m); transpose: of the transposed block; edge_grid: the grid rule of the edge
 *                arrays (else of the node arrays)
 *   q2r          n quaternions -> n blocks (q2R.m)
 *   edge_log     Q (n), QQ (m) -> B (m x 3), Weighted_LAA.m:9-35; the device problem must hold rotations (any)
 *   rhs          w (m), B (m x 3) -> rhs (n x 3), diag (n): A' W^2 B and the diagonal of A' W^2 A
 *   pcg          the Jacobi-PCG: w3 = 0 Weighted_LAA's instance (w: m, diag: n, probed every 25 steps), w3 = 1 the primal-dual Newton
 *                instance with breakdown tracking (w: 3m, diag: 3n, probed every 5 steps); act[3] selects the coordinates of the
 *                convergence test.  Out: x (n x 3), bad[3], the last probe's |r|^2 and |b|^2 per coordinate (rnorm[3], bnorm[3]) and
 *                the solve's bookkeeping (steps, 1 if it stopped at the cap, largest |r| / |b|)
 *   node_update  x (n x 3), Q (n) -> Q * exp(x), the vector parts Wv (n x 3) and sum_{v >= 1} |x_v| (Weighted_LAA.m:40-50; the
 *                library divides the sum by n); irls_node_update: the same with max_{v >= 1} |x_v| (BoxMedianSO3Graph.m:172-185)
 *   weights      x (m), thresh -> min(1 / x^0.75, 1e4), 1e-4 where x > thresh (DESC.m:298-303)
 *   irls_weights x (n x 3), B (m x 3) -> the GM / L12 weights of the edge residuals (mode: DESC_IRLS_GM / DESC_IRLS_L12)
 *   quantile     MATLAB's quantile(x, p) of m values; cap: most values collected from the two histogram bins before the exact
 *                host path takes over (the library passes 2^20)
 *   irls_project m blocks Rij (+ optional caller rows `order`) -> P = U round(S) V' of their transposes (m x 9), the smallest failing
 *                caller row (-1: none), the number of warned edges; only >= 0: also that edge's {status, det, s1, s2, s3} in info[5] */
int desc_test_laa_r2q(const double* R, int64_t count, int32_t transpose, int32_t edge_grid, int32_t device, double* Q);
int desc_test_laa_q2r(const double* Q, int64_t n, int32_t device, double* R);
int desc_test_laa_edge_log(const desc_device_problem* dp, const double* Q, const double* QQ, int64_t m, double* B);
int desc_test_laa_rhs(const desc_device_problem* dp, const double* w, const double* B, int64_t m, double* rhs, double* diag);
int desc_test_laa_pcg(const desc_device_problem* dp, int32_t w3, const double* w, const double* rhs, const double* diag, int64_t m,
                      const int32_t* act, double* x, int32_t* bad, double* rnorm, double* bnorm, int32_t* total, int32_t* unconverged,
                      double* worst);
int desc_test_laa_node_update(const double* x, const double* Q, int64_t n, int32_t device, double* Q_out, double* Wv, double* score);
int desc_test_irls_node_update(const double* x, const double* Q, int64_t n, int32_t device, double* Q_out, double* score);
int desc_test_laa_weights(const double* x, int64_t m, double thresh, int32_t device, double* w);
int desc_test_irls_weights(const desc_device_problem* dp, const double* x, const double* B, int64_t m, int32_t mode, double sigma,
                           double* w);
int desc_test_laa_quantile(const double* x, int64_t m, double p, int64_t cap, int32_t device, double* result);
int desc_test_irls_project(const double* rij, const int32_t* order, int64_t m, int64_t only, int32_t device, double* P,
                           int32_t* bad_row, int32_t* warn, double* info);

/* Test hooks (tests/test_gpu_pd_kernels.py, tests/test_gpu_pd_solver.py): the L1 stage's primal-dual solver (l1decode_pd, three
 * coordinates batched; irls.hip).  A NULL pointer, an m or n that is not the device problem's, an unknown stage or a negative pdmaxiter
 * returns DESC_ERR_INVALID before any device work.
 *   pd_stage  one kernel on a snapshot of the solver's whole state, launched as the solver launches it.  tau, s, ymax, act: the three
 *             coordinates' scalars of the launch (gather1 forms its coefficient -1 / tau, 0 for act = 0, as the solver does; gather2
 *             ignores them).  edge: 17 arrays of m x 3 in the order y Ax u fu1 fu2 lamu1 lamu2 w2 sig1 sig2 sigx ev1 ev2 Adx du dlamu1
 *             dlamu2; node: 6 arrays of n x 3 in the order x Atv w1p diag dx Atdv; part: 6 * 256 doubles, the block partials [256][K]
 *             (K = 3 absmax / resid, 6 dir / accept).  All three are uploaded, and every array comes back after the launch: what the
 *             kernel does not write returns with the bits it came with.
 *   pd_solve  the whole solver on B (m x 3) from x = 0.  x (n x 3); state: the final u, lamu1, lamu2, Ax (m x 3 each) and Atv (n x 3),
 *             12 m + 3 n doubles; counters[6]: steps, ill-conditioned returns, stuck returns, Newton solves, CG steps, CG solves stopped
 *             at the cap.  trace: trace_cap records of 3 x 8 doubles, record 0 the start, record k step k, per coordinate {takes
 *             part, the CG broke down, first trial step, trials, verdict (0 none, 1 accepted, 2 stuck), sdg, tau, resnorm after the
 *             step}; *trace_len: records written. */
enum { DESC_TEST_PD_ABSMAX = 0, DESC_TEST_PD_INIT, DESC_TEST_PD_GATHER0, DESC_TEST_PD_GATHER1, DESC_TEST_PD_GATHER2, DESC_TEST_PD_PRE,
       DESC_TEST_PD_DIR, DESC_TEST_PD_RESID, DESC_TEST_PD_RESID_TRIAL, DESC_TEST_PD_ACCEPT, DESC_TEST_PD_STAGES };
int desc_test_irls_pd_stage(const desc_device_problem* dp, int32_t stage, const double* tau, const double* s, const double* ymax,
                            const int32_t* act, int64_t m, int64_t n, double* edge, double* node, double* part);
int desc_test_irls_pd_solve(const desc_device_problem* dp, const double* B, int64_t m, int64_t n, int32_t pdmaxiter, double* x,
                            double* state, int32_t* counters, double* trace, int32_t trace_cap, int32_t* trace_len);

/* Test hooks (tests/test_gpu_spectral_kernels.py, tests/test_spectral_host.py): the kernels of the Spectral / GCW eigen-solve
 * (spectral.hip) one at a time on caller (host) arrays, and the small dense helpers it shares with the batched solve (small_dense.h).
 * Each launches through the function the product path launches with; grid = 0 is the product path's grid rule, another value forces
 * that many workgroups (so that the stride loops turn at small sizes).  A NULL pointer, a negative count, an m that is not the device
 * problem's, an unknown form or a grid outside [0, 65535] returns DESC_ERR_INVALID before any device work.
 *   weights    S (m) -> 1 / (S^1.5 + 1e-8)  (GCW.m:20)
 *   row_wsum   w (m; NULL: ones) -> the weighted degree of every node (n)
 *   assemble   w (m; NULL: ones), dinv (n; NULL: ones) -> the 2m blocks as stored: 18 m doubles, component-major
 *              (blocks[q * 2m + t], q = r + 3k of CSR slot t)
 *   spmm       y = alpha A x + s1 x + s2 z for the given blocks; x, z, y: 3n x 6 row-major.  form 0: the product path's choice between
 *              the wave-per-row (64) and workgroup-per-row (256) kernels, 64 / 256: that one, 2: the v_mfma_f64_4x4x4 form (refused
 *              unless the operand layout probe agrees).  z_is_y: launched with z aliasing y
 *   gram       X, Y (rows x 6) -> G1 = X'Y, G2 = Y'Y (6 x 6 row-major), the host sum over the workgroups' partials included
 *   residual   X, Y (rows x 6), Z3 (6 x 3 row-major: the three Ritz vectors' coefficients), theta (3) -> r2[c] = |Y z_c - theta_c X z_c|^2
 *   combine    Y (rows x 6), C (6 x 6 row-major) -> Y C
 *   small_jacobi   N = 3 or 6: symmetric A (N x N) -> eigenvalues w descending, eigenvectors in the columns of V
 *   small_ortho    G, Z (6 x 6; Z NULL: identity) -> C = Z L^-T with Z'GZ = L L'; *ok = 0 where that is not positive definite
 *   small_project  count 3x3 blocks M (row-major) -> their projections onto SO(3) (row-major)
 *   small_ritz_tail  V (3n x 3 Ritz vectors), dinv (n; NULL: none) -> scaling, sign fix and per-node projection, R_out 3x3xn column-major
 * The small_* hooks are host code only. */
int desc_test_spectral_weights(const double* S, int64_t m, int32_t device, double* w);
int desc_test_spectral_row_wsum(const desc_device_problem* dp, const double* w, int64_t m, int32_t grid, double* deg);
int desc_test_spectral_assemble(const desc_device_problem* dp, const double* w, const double* dinv, int64_t m, int32_t grid, double* blocks);
int desc_test_spectral_spmm(const desc_device_problem* dp, const double* blocks, const double* x, const double* z, int32_t z_is_y,
                            int32_t form, int32_t grid, double alpha, double s1, double s2, double* y);
int desc_test_spectral_gram(const double* X, const double* Y, int64_t rows, int32_t grid, int32_t device, double* G1, double* G2);
int desc_test_spectral_residual(const double* X, const double* Y, int64_t rows, const double* Z3, const double* theta, int32_t grid,
                                int32_t device, double* r2);
int desc_test_spectral_combine(const double* Y, int64_t rows, const double* C, int32_t grid, int32_t device, double* Xn);
int desc_test_small_jacobi(int32_t N, const double* A, double* w, double* V);
int desc_test_small_ortho(const double* G, const double* Z, double* C, int32_t* ok);
int desc_test_small_project(const double* M, int64_t count, double* R);
int desc_test_small_ritz_tail(const double* V, const double* dinv, int64_t n, double* R_out);

#ifdef __cplusplus
}
#endif
#endif /* DESC_AMD_H */

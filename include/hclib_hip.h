/*
 * hclib_hip.h — the MI355X `modules/hip` C ABI.
 *
 * HClib's plug-in ABI lets a module add a locale type and run work there
 * (inc/hclib-module.h:62-106, src/hclib_module.c:49-160). The reference's
 * only device module, modules/cuda, runs kernels from CPU tasks and polls
 * for completion (modules/cuda/inc/hclib_cuda.h:21-74). This module instead
 * moves the scheduler itself onto the GPU: every entry point below replaces
 * a piece of the reference's CPU hot path with a hand-written gfx950 kernel.
 *
 *   entry point                      replaces (reference file:line)
 *   -------------------------------  -------------------------------------------
 *   hclib_hip_forasync1d/2d/3d       hclib_forasync + forasync{1,2,3}D_{flat,
 *                                    recursive,runner}  src/hclib.c:110-464
 *   hclib_hip_forasync_triad_f32     the forasync1D_runner loop of a triad body
 *                                    src/hclib.c:110-120 (BASELINE config 1)
 *   hclib_hip_uts_search             core_work_loop/find_and_run_task/deque_*
 *                                    src/hclib-runtime.c:646-729,
 *                                    src/hclib-deque.c:50-139, driving the UTS
 *                                    tasks of test/uts/UTS.cpp:154-232
 *   hclib_hip_fib                    spawn/finish counters of test/fib/fib.c:57-71
 *                                    (async/finish) and 113-141 (DDT), i.e.
 *                                    src/hclib-runtime.c:431-446, 572-617,
 *                                    1219-1277
 *   hclib_hip_sw                     promise put / waiter release of
 *                                    src/hclib-promise.c:132-245 driving the tile
 *                                    DAG of test/smithwaterman/smith_waterman.cpp
 *                                    :119-239
 *   hclib_hip_dag_*                  the same dependency-counter release for any
 *                                    async_await DAG built through hclib.h
 *   hclib_hip_cholesky               the k-loop and its two finish scopes per step
 *                                    of test/cholesky/cholesky.cpp:80-124, with the
 *                                    four tile kernels, as one promise-DAG launch
 *   hclib_hip_sort_i64               the spawns, the finish scopes with dynamic
 *                                    check-in (src/hclib-runtime.c:431-446) and the
 *                                    leaves of BOTS sort, test/performance-regression/
 *                                    full-apps/bots/sort/sort.ref.c:315-423, as one
 *                                    launch of dynamic device dataflow
 *   hclib_hip_sparselu               the kk loop and its two finish barriers per step
 *                                    of BOTS sparselu (bots/sparselu_single/
 *                                    sparselu.c:331,348; sparselu.ref.c:300-322) with
 *                                    its four block kernels, as one promise-DAG
 *                                    launch whose graph a symbolic pass over the
 *                                    block mask builds
 *   hclib_hip_nqueens                the asyncs, the finish per call and the csols[]
 *                                    sums of BOTS nqueens (bots/nqueens/nqueens.c:
 *                                    125-182), and the flat form's asyncs and counter
 *                                    (full-apps/nqueens.cpp:41-60), as task kinds of
 *                                    the work-stealing megakernel
 *   hclib_hip_strassen               the seven asyncs, their finish scopes and the
 *                                    taskwait of BOTS strassen (bots/strassen/
 *                                    strassen.c, strassen.ref.c:580-788), the two
 *                                    sweeps as band tasks, as one launch of dynamic
 *                                    device dataflow
 *   hclib_hip_health                 the task per village, the taskwait and the
 *                                    sim_time loop of BOTS health (bots/health/
 *                                    health.ref.c:426-461, 567-586; health.c:421-466)
 *                                    with its five list walks as wave-wide
 *                                    partitions, every round of the same fork-join
 *                                    tree in one launch of dynamic device dataflow
 *   hclib_hip_floorplan              the async per (shape, corner) candidate, the
 *                                    pruning against MIN_AREA and the critical
 *                                    section of BOTS floorplan (bots/floorplan/
 *                                    floorplan.c:230-328), as a task kind of the
 *                                    work-stealing megakernel with the bound as one
 *                                    word every XCD reads and lowers
 *   hclib_hip_alignment              the hclib_start_finish and its hclib_async per
 *                                    sequence pair of BOTS alignment (bots/
 *                                    alignment_for, alignment_single: alignment.c;
 *                                    the algorithm alignment.ref.c:204-529), the two
 *                                    halves of Myers-Miller's diff as further tasks,
 *                                    every sweep a wave-wide task body, as one launch
 *                                    of dynamic device dataflow
 *   hclib_hip_fft                    the three taskwaits of BOTS fft's fft_aux
 *                                    (bots/fft/fft.c, fft.ref.c:4653-4747) as finish
 *                                    scopes and continuations, the unshuffle and
 *                                    twiddle sweeps as band tasks, the r asyncs as
 *                                    child tasks, as one launch of dynamic device
 *                                    dataflow
 *   hclib_hip_jacobi                 the copy and compute phases of Kastors jacobi's
 *                                    sweep() and the hclib_end_finish after each
 *                                    (kastors-1.1/jacobi/src/jacobi-block-task.c:
 *                                    57-108), as neighbour awaits between block
 *                                    tasks of consecutive (time-fused) sweeps in
 *                                    one launch of the device promise DAG
 *   hclib_hip_bfs                    the two hclib_forasync_future sweeps per level
 *                                    and the hclib_future_wait after each of
 *                                    Rodinia bfs (rodinia/bfs/bfs.cpp; bfs.ref.cpp:
 *                                    139-182), as frontier items of the
 *                                    work-stealing megakernel whose last finisher
 *                                    opens the next level
 *   hclib_hip_cfd                    the 41 hclib_forasync_future sweeps of Rodinia
 *                                    cfd and the hclib_future_wait after each
 *                                    (rodinia/cfd/euler3d_cpu_double.cpp:74-79,
 *                                    147-152, 228-233, 294-299, 460-465; the loop
 *                                    euler3d_cpu_double.ref.cpp:470-482), as awaits
 *                                    between (stage, block) tasks read off the
 *                                    mesh, in one launch of the device promise DAG
 *   hclib_hip_srad                   the host thread's sums over the region of
 *                                    interest and the two hclib_forasync_future
 *                                    sweeps of Rodinia srad with the
 *                                    hclib_future_wait after each (rodinia/srad/
 *                                    srad.cpp; srad.ref.cpp:131-207), as one reduce
 *                                    task whose promise carries q0sqr and one task
 *                                    per block and iteration that awaits it, in one
 *                                    launch of the device promise DAG
 *   hclib_hip_atomic_*,            the per-thread copies and the gather of
 *   hclib_hip_forasync_reduce        inc/hclib_atomic.h:37-42, 81-186 and
 *                                    src/hclib_atomic.c:34-54, one slot per wave
 *
 * Conventions (mirroring the reference's error behaviour):
 * plain pointers and sizes only; functions return 0 on success and a
 * negative HCLIB_HIP_E* code on failure, with a message retrievable via
 * hclib_hip_last_error(). Device-side failures (queue overflow, bounded
 * spins that time out) set a device error word that the host checks after
 * every launch. Nothing here ever falls back to the CPU: without a usable
 * gfx950 device every compute entry point fails with HCLIB_HIP_ENODEV.
 */
#ifndef HCLIB_HIP_H_
#define HCLIB_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HCLIB_HIP_OK 0
#define HCLIB_HIP_ENODEV (-1)   /* no HIP device / not gfx950 */
#define HCLIB_HIP_EINVAL (-2)   /* bad arguments */
#define HCLIB_HIP_ENOMEM (-3)   /* device allocation failed */
#define HCLIB_HIP_EDEVICE (-4)  /* device-side error word set (see message) */
#define HCLIB_HIP_EHIP (-5)     /* a HIP runtime call failed */

/* ---------------------------------------------------------------- module */
/* hclib_hip_init: bind the calling process to HIP device `device` (the
 * module's post-init hook, inc/hclib-module.h:62-64). Idempotent. */
int hclib_hip_init(int device);
/* hclib_hip_finalize: wait for the module stream and free every device
 * allocation the library holds on its own account; hclib_hip_init (of any
 * device) starts again from nothing. Handles the caller owns (atomics, SW band
 * sessions, global regions, locale allocations, forasync op records) stay the
 * caller's to release. */
void hclib_hip_finalize(void);
/* out[0] = live device allocations, out[1] = their bytes, of the library's own
 * account (its arenas and per-call buffers; not the caller-owned handles
 * above): {0, 0} after hclib_hip_finalize */
void hclib_hip_device_memory_live(uint64_t out[2]);
const char *hclib_hip_last_error(void);
/* Number of CUs / XCDs of the bound device (0 if none). */
int hclib_hip_num_cus(void);
/* the bound device (-1 before hclib_hip_init) and the module's HIP stream
 * (NULL before): what the hip plug-in module's memory callbacks run on */
int hclib_hip_device(void);
void *hclib_hip_stream(void);
/* Module version string, also proves the library loads without a GPU. */
const char *hclib_hip_version(void);
/* Scheduler counters of the last megakernel launch (HCLIB_STATS analogue,
 * src/hclib-runtime.c:83-104): [0..1] kind totals, [7..8] diagnostic phase
 * cycles (HCLIB_HIP_STAMPS=1), [9] busy, [10] idle, [11] spill cycles,
 * [12] waves, [13] batches, [14] chunks pushed, [15] chunks stolen. */
void hclib_hip_last_sched_counters(uint64_t out[16]);

/* Per-wave records of the last megakernel launch (the per-worker lines of
 * HCLIB_STATS, src/hclib-runtime.c:1370-1410): each wave writes its own
 * record as it leaves. Summed over the waves, batches / chunks_pushed /
 * chunks_stolen equal hclib_hip_last_sched_counters [13] / [14] / [15].
 * Copies at most `max` records to out; returns the number of waves. */
typedef struct {
    uint64_t executed;      /* tasks run (one lane of a batch each) */
    uint64_t spawned;       /* children created */
    uint64_t batches;
    uint64_t chunks_pushed; /* chunks given to the HBM deques */
    uint64_t chunks_stolen; /* chunks taken from a deque other than the wave's home deque */
    uint64_t items_stolen;  /* tasks in those chunks */
    uint64_t xcd;           /* the XCD the wave ran on */
    uint64_t reserved;
    uint64_t stolen_from[8]; /* chunks taken from each XCD's deques */
} hclib_hip_wave_stats_t;
int hclib_hip_last_wave_stats(hclib_hip_wave_stats_t *out, int max);
/* The narrow-frontier carry loop of the last launch (hx_sched.h): [0]
 * batches run in it, [1] shader-clock cycles spent in it, [2] entries. */
void hclib_hip_last_narrow_counters(uint64_t out[4]);
/* That loop's overflow exits in workgroups with sibling waves (a level that
 * outgrew one batch; hx_sched.h narrow_shed; zeros with HCLIB_HIP_NARROW_SHED=0):
 * [0] exits, [1] exits whose shed children all went to idle siblings' LDS
 * inboxes (the loop went on), [2] inboxes filled, [3] items in them, [4]
 * exits that left children for the ring and the main loop; [0] = [1] + [4]. */
void hclib_hip_last_shed_counters(uint64_t out[8]);
/* The hand-off waves of the last megakernel launch (hx_sched.h comm_wave; UTS
 * BIN workgroups with HCLIB_HIP_UTS_COMM != 0, zeros otherwise): [0] outbox
 * blocks filled by the main loop's give-away, [1] items in them, [2] outbox
 * blocks filled by the narrow loop's overflow exit, [3] items in them, [4]
 * blocks the hand-off waves enqueued to an HBM deque, [5] blocks they copied
 * to a sibling that had gone idle ([0] + [2] = [4] + [5]), [6] give-aways and
 * exits that found no outbox free, [7] overflow exits that still left
 * children for the ring. */
void hclib_hip_last_comm_counters(uint64_t out[8]);
/* Diagnostic (HX_PHASES builds, zeros otherwise): [0] main-loop single
 * batches of the last megakernel launch, [1..4] their s_memtime cycles from
 * loop top to pop issued, pop landed, body done, batch end. */
void hclib_hip_last_phase_counters(uint64_t out[8]);
/* Worker timelines of the last megakernel launch (diagnostic: a library
 * built with `--variant timeline` and HCLIB_HIP_TIMELINE=<events per
 * worker>; hx_sched.h Timeline). Copies at most `max_words` events (worker w's
 * at [w * events_per_worker ...], 0 = unused) and returns the worker count
 * (0 when no timeline was recorded). */
int hclib_hip_last_timeline(uint64_t *out, uint64_t max_words, uint32_t *events_per_worker);

/* L2 atomic-throughput calibration: the saturated rate (million atomic
 * ops per second, whole GPU) of one access shape the runtime's atomics use,
 * the "peak" fib/SW/scheduler atomic rates are priced against.
 *   0 HCLIB_HIP_ATOMIC_SCATTER_RET64: every lane a returning 64-bit add on
 *     its own random 16-B record (fib join check-out, SW dependency counters)
 *   1 HCLIB_HIP_ATOMIC_HOT_WORD: lane 0 of every wave on ONE shared word
 *     (deque tickets, the `outstanding` termination counter)
 *   2 HCLIB_HIP_ATOMIC_COALESCED32: 64 consecutive non-returning 32-bit adds
 *     per wave instruction (the L2 atomic units' streaming peak)
 * `iters` atomic ops per lane (mode 1: per wave). */
#define HCLIB_HIP_ATOMIC_SCATTER_RET64 0
#define HCLIB_HIP_ATOMIC_HOT_WORD 1
#define HCLIB_HIP_ATOMIC_COALESCED32 2
int hclib_hip_atomic_calibrate(int mode, int iters, double *mops_per_s, double *kernel_ms);
/* SparseLU calibration (not part of the factorisation's API): the bmod body of
 * hclib_hip_sparselu alone, `reps` times per workgroup on resident B x B
 * blocks, wgs_per_cu (1 or 2) workgroups per CU: kernel ms and the unfused f32
 * rate (2 B^3 operations per bmod) the factorisation's updates can reach. */
int hclib_hip_sparselu_bmod_rate(int B, int wgs_per_cu, int reps, double *ms, double *gflops);
/* The chip's UTS SHA-1 issue ceiling: `chains` (1 or 2) independent rng_spawn
 * chains per lane (the instruction stream k_uts_search runs per node),
 * waves_per_cu waves on every CU, `iters` spawns per chain; SHA-1
 * compressions per second over the timed launch (the peak of the UTS
 * kernel's VALU roofline; bench.py `roofline_uts`). */
int hclib_hip_sha1_calibrate(int chains, int waves_per_cu, int iters, double *sha1_per_s, double *kernel_ms);

/* ----------------------------------------------- user device task kinds */
/* The persistent-megakernel scheduler for task kinds compiled in the
 * caller's own HIP translation unit (include/hclib_hip_cpp.h,
 * hclib::hip::run_tasks<Kind>): begin() carves and resets the chunk deques
 * for `entry_words` u32 per queued item, resets the scheduler globals and
 * records the start event on the module stream; the caller launches
 * `grid` workgroups of 64 threads on `stream`; end() records the stop
 * event, waits, and returns the counters (see hclib_hip_last_sched_counters)
 * and the device error, if any, as HCLIB_HIP_EDEVICE. */
typedef struct {
    void *hdr;         /* deque headers */
    uint32_t *seq;     /* per-slot sequence words */
    uint32_t *cnt;     /* per-slot item counts */
    uint32_t *data;    /* chunk payloads */
    uint32_t nq, cap, chunk;
    void *globals;     /* scheduler globals (device) */
    void *stream;      /* hipStream_t of the module */
    int grid;          /* workgroups (waves) to launch */
    int num_cus;
} hclib_hip_sched_launch_t;

int hclib_hip_sched_begin(uint32_t entry_words, uint32_t chunk, int waves_per_cu,
                          hclib_hip_sched_launch_t *out);
int hclib_hip_sched_end(const char *who, uint64_t counters[16], uint64_t maxes[4],
                        double *kernel_ms);

/* ------------------------------------------------------------ forasync */
/* hclib_loop_domain_t of inc/hclib-task.h:53-58 (int bounds, 16 bytes). */
typedef struct {
    int low;
    int high;
    int stride;
    int tile;
} hclib_hip_loop_domain_t;

#define HCLIB_HIP_FORASYNC_FLAT 0      /* FORASYNC_MODE_FLAT, inc/hclib.h:161 */
#define HCLIB_HIP_FORASYNC_RECURSIVE 1 /* FORASYNC_MODE_RECURSIVE, inc/hclib.h:159 */

/* Device loop bodies. A host function pointer cannot run on the GPU, so a
 * forasync at the GPU locale names one of these registered body kinds. */
#define HCLIB_HIP_BODY_TRIAD_F32 1 /* a[i] = b[i] + s*c[i] (1-D) */
#define HCLIB_HIP_BODY_IOTA_CHECK 2 /* assert(ran[i]==-1); ran[i]=i, as test/c/forasync1DCh.c:45-49 (1-D) */
#define HCLIB_HIP_BODY_VISIT_COUNT 3 /* counts[linear(i,j,k)] += 1 (1/2/3-D) */

typedef struct {
    float *a;
    const float *b;
    const float *c;
    float s;
} hclib_hip_triad_args_t;

typedef struct {
    int *ran;      /* device pointer, indexed by i */
    int *errors;   /* device pointer to one int: number of failed checks */
} hclib_hip_iota_args_t;

typedef struct {
    int *counts;   /* device pointer */
    int base[3];   /* index origin per dim */
    int extent[3]; /* counts has extent[0]*extent[1]*extent[2] ints, row-major */
} hclib_hip_visit_args_t;

/* hclib_forasync (src/hclib.c:452-464) for dim in 1..3 at the GPU locale.
 * `domain` has `dim` entries; tile == -1 is replaced by
 * ceil((high-low)/nworkers) with nworkers = the module's worker count (the
 * number of resident waves, hclib_hip_num_workers()) and written back, as
 * the reference does. The iteration set is exactly the reference's for the
 * given mode (including the FLAT 1-D quirk of src/hclib.c:322-337).
 * `args` points to the body's argument struct (host memory, copied by
 * value). `stream` is a hipStream_t (NULL = default). Asynchronous: the
 * call returns after enqueueing; synchronize on the stream. */
int hclib_hip_forasync(int body, const void *args, int dim, hclib_hip_loop_domain_t *domain,
                       int mode, void *stream);

/* Fast path of hclib_hip_forasync for the triad over [0, n): coalesced
 * grid-stride float4 tiles, no FMA contraction (bit-exact with the CPU). */
int hclib_hip_forasync_triad_f32(float *a, const float *b, const float *c, float s, int64_t n,
                                 void *stream);

/* Resident worker waves the forasync/megakernel launches use. */
int hclib_hip_num_workers(void);

/* The iteration set of hclib_hip_forasync, for device loop bodies compiled
 * in the caller's own HIP translation unit (hclib::hip::forasync_device in
 * include/hclib_hip_cpp.h): plan() applies the reference's tiling (tile ==
 * -1 written back as in hclib_hip_forasync; FLAT and RECURSIVE sets exactly
 * as src/hclib.c:110-464 enumerate them) and uploads one table of runs per
 * dimension in `stream` order; iteration t of the sweep (0 <= t < total,
 * innermost dimension fastest) maps to (i, j, k) through the runs. release()
 * frees the tables in stream order after the sweep. */
typedef struct {
    int first, count, stride, pad;  /* indices first + m * stride, m < count */
} hclib_hip_run_t;
typedef struct {
    const hclib_hip_run_t *runs[3];
    const int64_t *prefix[3];  /* prefix[d][r] = iterations of dimension d before run r */
    int nruns[3];
    int ndim;
    int64_t total;
    void *mem;
} hclib_hip_sweep_plan_t;
int hclib_hip_forasync_plan(int dim, hclib_hip_loop_domain_t *domain, int mode, void *stream,
                            hclib_hip_sweep_plan_t *plan);
int hclib_hip_forasync_plan_release(hclib_hip_sweep_plan_t *plan, void *stream);

/* ---------------------------------------------------- privatised atomics */
/* The device form of inc/hclib_atomic.h (hclib_atomic_t and the C++
 * atomic_sum_t / atomic_max_t / atomic_or_t, inc/hclib_atomic.h:37-42,
 * 141-186): one padded slot per worker, updated without contention and folded
 * on request. A device worker is a wave; device code updates through
 * hx::AtomicView (include/hclib_hip/hx_atomic.h), the host creates, gathers
 * and resets through the calls below.
 *
 * create   allocates nslots slots of HCLIB_HIP_ATOMIC_STRIDE bytes (nslots: a
 *          power of two >= the worker count of every launch this library
 *          makes) plus one result word, and resets them. `default_value`
 *          points to one value of `dtype`. MAX and OR start every slot at the
 *          default; SUM starts every slot at zero and adds the default once
 *          at the gather (nslots copies of a non-zero default must not be
 *          summed), so an atomic always reads its default after a reset. OR
 *          is the reference's logical or: the result is 0 or 1.
 * view     fills the struct device code is handed (by value).
 * gather   one workgroup folds the slots in a fixed tree order into the
 *          result word, in `stream` order; the call then copies the word to
 *          host_out (one value of dtype) and waits. Gather does not reset:
 *          updates of successive launches accumulate, as the reference's
 *          gather leaves the per-thread copies alone (src/hclib_atomic.c:40-54).
 * gather_async  the same fold into device memory `device_out`, no wait.
 * reset    every slot back to its start value, in `stream` order.
 * destroy  waits for the device, then frees. */
#define HCLIB_HIP_ATOMIC_I32 0
#define HCLIB_HIP_ATOMIC_U32 1
#define HCLIB_HIP_ATOMIC_I64 2
#define HCLIB_HIP_ATOMIC_U64 3
#define HCLIB_HIP_ATOMIC_F32 4
#define HCLIB_HIP_ATOMIC_F64 5
#define HCLIB_HIP_ATOMIC_SUM 0
#define HCLIB_HIP_ATOMIC_MAX 1
#define HCLIB_HIP_ATOMIC_OR 2
#define HCLIB_HIP_ATOMIC_STRIDE 128 /* bytes between slots: one L2 line each */

typedef struct hclib_hip_atomic hclib_hip_atomic_t;
typedef struct {
    void *slots;     /* device pointer to slot 0 */
    uint32_t nslots; /* power of two */
    uint32_t stride; /* bytes between slots */
    int dtype, op;
} hclib_hip_atomic_view_t;

int hclib_hip_atomic_create(int dtype, int op, const void *default_value, hclib_hip_atomic_t **out);
int hclib_hip_atomic_destroy(hclib_hip_atomic_t *atomic);
int hclib_hip_atomic_view(const hclib_hip_atomic_t *atomic, hclib_hip_atomic_view_t *view);
int hclib_hip_atomic_gather(hclib_hip_atomic_t *atomic, void *stream, void *host_out);
int hclib_hip_atomic_gather_async(hclib_hip_atomic_t *atomic, void *stream, void *device_out);
int hclib_hip_atomic_reset(hclib_hip_atomic_t *atomic, void *stream);

/* A reducing forasync with the built-in body `update(x[i])`: x is a device
 * array of the atomic's dtype, indexed by the iterations of the 1-D `domain`
 * (dim must be 1) exactly as hclib_hip_forasync enumerates them for `mode`
 * (tile == -1 resolved and written back likewise). Every thread keeps its
 * partial value in a register, every wave updates its slot once. One
 * unit-stride run is read with 16-byte loads (alignment prologue and tail
 * included); any other set goes through the run tables. Asynchronous on
 * `stream`; read the value with hclib_hip_atomic_gather. */
int hclib_hip_forasync_reduce(hclib_hip_atomic_t *atomic, const void *x, int dim, hclib_hip_loop_domain_t *domain,
                              int mode, void *stream);

/* ----------------------------------------------------------------- UTS */
/* Tree parameters: the UTS CLI flags of test/uts/uts.c:380-420 (same field
 * order as oracle/uts_oracle.h so both sides read the same struct). */
typedef struct {
    int type;         /* -t: 0 BIN, 1 GEO, 2 HYBRID, 3 BALANCED */
    int shape_fn;     /* -a: 0 LINEAR, 1 EXPDEC, 2 CYCLIC, 3 FIXED */
    int gen_mx;       /* -d */
    int root_id;      /* -r */
    int non_leaf_bf;  /* -m */
    int compute_gran; /* -g */
    double b_0;       /* -b */
    double non_leaf_prob; /* -q */
    double shift_depth;   /* -f */
} hclib_hip_uts_params_t;

typedef struct {
    uint64_t nodes;     /* tree size   (UTS.cpp:241, uts.c:462) */
    uint64_t leaves;    /* num leaves */
    uint64_t max_depth; /* tree depth */
    uint64_t chunks_pushed;  /* work chunks spilled to the HBM deques */
    uint64_t chunks_stolen;  /* chunks taken from another worker's deque */
    uint64_t batches;        /* wave batches executed */
    double kernel_ms;        /* device time of the search launch (HIP events) */
    double busy_frac;        /* share of wave time spent inside batches */
    double us_per_batch;     /* average wave time per batch (incl. spills) */
} hclib_hip_uts_result_t;

/* Search the whole tree on the bound GPU (persistent megakernel: per-wave
 * LDS stacks, per-XCD chunk deques in HBM, device-atomic stealing,
 * outstanding-work termination). Multi-GPU sharding: with nshards > 1 every
 * shard expands the levels above split_depth identically (counted by shard
 * 0 only); shard `shard` keeps the depth-split_depth nodes whose first state
 * word is congruent to shard (mod nshards) and searches their subtrees.
 * Per-shard results sum to the whole tree (max for depth); with a global
 * region attached (hclib_hip_global_*) subtrees below the split also move
 * between shards. level_hist (host, may be NULL) receives nodes per depth
 * for depth < max_levels (max_levels <= 65536). */
int hclib_hip_uts_search(const hclib_hip_uts_params_t *params, int shard, int nshards,
                         int split_depth, hclib_hip_uts_result_t *result, uint64_t *level_hist,
                         int max_levels);

/* The launch shape hclib_hip_uts_search chose for its last search on this
 * thread's module (diagnostic: tests pin the bench's exact configuration).
 * mode: 0 rule tables in global memory, 1 in LDS, 2 BIN, 3 fixed-shape GEO;
 * feat: 0 the plain kernel, 1 sharding / per-level counts, 2 depth trace;
 * seeded: breadth-first seeding of the top levels (seed_target slots). */
typedef struct {
    int mode, feat, workers_per_group, grid, ring, seeded, seed_target, spill_lo, waves_per_cu;
} hclib_hip_uts_launch_t;
int hclib_hip_uts_last_launch(hclib_hip_uts_launch_t *out);

/* Cross-GPU work sharing for sharded searches (one process per GPU;
 * SURVEY 8e items 2-3; the reference's distributed UTS moves work between
 * ranks, test/performance-regression/full-apps/uts/uts_hclib_shmem_opt.cpp
 * :98-140). One region of hclib_hip_global_bytes(cap) bytes lives in one
 * rank's device memory; the other ranks map it with hclib_hip_ipc_import
 * (handle from hclib_hip_ipc_export: HIP_IPC_HANDLE_SIZE = 64 bytes). Before
 * each sharded launch one rank resets it (hclib_hip_global_init, nranks =
 * ranks that will launch) and every rank waits for that (a barrier); a rank
 * that attached it (hclib_hip_global_attach, NULL detaches) then shares
 * work in every sharded hclib_hip_uts_search: idle waves take chunks from
 * the region's ring, busy waves export chunks while some rank is idle, and
 * each rank's launch ends only when no rank holds work (the region's
 * `active` count, system-scope atomics). hclib_hip_global_read fills
 * out[0] active, out[1] idle ranks, out[2] chunks queued, then per rank r
 * out[3 + 2r] chunks exported and out[4 + 2r] chunks imported (r < 16).
 * hclib_hip_global_alloc allocates the region itself (kind 0 uncached device
 * memory, 1 fine-grained, 2 plain hipMalloc; free with hclib_hip_global_free)
 * so that its IPC handle names exactly that allocation. */
size_t hclib_hip_global_bytes(uint32_t cap);
int hclib_hip_global_alloc(uint32_t cap, int kind, void **region_out);
int hclib_hip_global_free(void *region);
int hclib_hip_global_init(void *region, uint32_t cap, int nranks);
int hclib_hip_global_attach(void *region, uint32_t cap, int rank);
int hclib_hip_global_read(const void *region, uint64_t out[35]);
int hclib_hip_ipc_export(void *dev_ptr, void *handle_out);
int hclib_hip_ipc_import(const void *handle, void **dev_ptr_out);
int hclib_hip_ipc_close(void *dev_ptr);

/* Host-side helper (no GPU needed): evaluate the integer numChildren rule
 * the device uses (threshold tables built from the reference's libm
 * formula, uts.c:171-274) for an explicit node; lets the CPU tests check
 * the tables against the oracle. st = the 5 big-endian state words. */
/* Host check (no GPU) of the device's bucketed numChildren lookup for
 * fixed-shape GEO trees: returns the number of rand values where the bucket
 * method disagrees with #{k : thr[k] <= rand} (0), checking every threshold
 * +-3, every bucket edge +-1 and `nrandom` pseudo-random values; *checked =
 * values compared (0 for trees without a threshold table). */
int hclib_hip_uts_bucket_check(const hclib_hip_uts_params_t *params, uint64_t nrandom, uint64_t *checked);
int hclib_hip_uts_num_children_host(const hclib_hip_uts_params_t *params, int height,
                                    const uint32_t st[5]);

/* ----------------------------------------------------------------- fib */
typedef struct {
    uint64_t tasks;      /* fib tasks executed (each fib(n) call is one task) */
    uint64_t joins;      /* finish scopes closed (join counters reaching 0) */
    uint64_t chunks_pushed;
    uint64_t chunks_stolen;
    double kernel_ms;
    double busy_frac;        /* share of wave time spent inside batches */
} hclib_hip_fib_result_t;

/* fib(n) with one task per call and a join counter per finish scope
 * (continuation by the last arriver). n <= 80. */
int hclib_hip_fib(int n, int64_t *value, hclib_hip_fib_result_t *result);

/* ---------------------------------------------- device promise DAG */
/* Device promises/futures with dependency-counter release
 * (include/hclib_hip/hx_dag.h; replaces hclib_promise_put's waiter walk,
 * src/hclib-promise.c:132-245, and spawn_await, src/hclib-runtime.c:596-644,
 * for device tasks). The caller describes `ntasks` tasks, each with
 * `payload_words` u32 of payload and the promises it awaits (CSR:
 * await_off[ntasks + 1], await_ids), and the promises already put before the
 * launch (preput[p] != 0, their datum in preput_datum; either may be NULL).
 * begin() uploads the graph, sizes every task's dependency counter, seeds
 * the ready list with the tasks that wait on nothing and records the start
 * event; the caller launches `grid` workgroups of 64 threads on `stream`
 * running hx::run_dag_worker<Kind> over `view` (hclib::hip::run_dag does
 * both); end() waits, copies each promise's datum / satisfied flag back
 * (either output may be NULL) and returns HCLIB_HIP_EDEVICE for a double put
 * or a task nothing releases (bounded spin, the reference's end_finish
 * deadlock). */
typedef struct {
    void *view;        /* hx::DagView (device pointers, by value) */
    void *stream;      /* hipStream_t of the module */
    int grid;          /* workgroups (waves) to launch */
    uint32_t ntasks, npromises;
} hclib_hip_dag_launch_t;

typedef struct {
    uint64_t tasks;      /* tasks executed */
    uint64_t puts;       /* device puts */
    uint64_t releases;   /* counter decrements that made a task ready */
    double kernel_ms;
} hclib_hip_dag_stats_t;

int hclib_hip_dag_begin(uint32_t ntasks, uint32_t npromises, uint32_t payload_words,
                        const uint32_t *payload, const uint32_t *await_off, const uint32_t *await_ids,
                        const uint8_t *preput, const uint64_t *preput_datum, int waves_per_cu,
                        uint32_t spin_limit_ms, hclib_hip_dag_launch_t *out);
int hclib_hip_dag_end(const char *who, uint64_t *datum_out, uint8_t *satisfied_out,
                      hclib_hip_dag_stats_t *stats);

/* ------------------------------------------ dynamic device dataflow */
/* Device tasks that create promises and async_await tasks while the launch
 * runs (include/hclib_hip/hx_dyn.h; hclib_promise_create / put and
 * spawn_await of src/hclib-promise.c:55-245, src/hclib-runtime.c:596-644 as
 * running tasks use them). begin() allocates the pools — task_cap tasks of
 * payload_words u32 each, promise_cap promises, node_cap wait nodes (one per
 * registered future) — seeds the ready list with the `nroots` root tasks
 * (payloads in root_payload) and records the start event; the caller
 * launches `grid` workgroups of 64 threads on `stream` running
 * hx::run_dyn_worker<Kind> over `view` (hclib::hip::run_dyn does both);
 * end() waits and returns HCLIB_HIP_EDEVICE for a double put, an exhausted
 * pool or tasks that wait on promises nothing puts (bounded spin, the
 * reference's end_finish deadlock). datum() then reads promises back. */
typedef struct {
    void *view;    /* hx::DynView (device pointers, by value) */
    void *stream;  /* hipStream_t of the module */
    int grid;      /* workgroups (waves) to launch */
} hclib_hip_dyn_launch_t;

typedef struct {
    uint64_t tasks;     /* tasks run (roots included) */
    uint64_t created;   /* tasks created by device async_await */
    uint64_t puts;      /* device puts */
    uint64_t releases;  /* waiters a put made runnable */
    uint64_t promises;  /* promises created on the device */
    double kernel_ms;
} hclib_hip_dyn_stats_t;

int hclib_hip_dyn_begin(uint32_t payload_words, const uint32_t *root_payload, uint32_t nroots, uint32_t task_cap,
                        uint32_t promise_cap, uint32_t node_cap, int waves_per_cu, uint32_t spin_limit_ms,
                        hclib_hip_dyn_launch_t *out);
int hclib_hip_dyn_end(const char *who, hclib_hip_dyn_stats_t *stats);
/* finish scopes of the last ended launch (hx::dyn_finish_open / _check_in /
 * _check_out, the reference's finish counter with dynamic check-in,
 * src/hclib-runtime.c:431-446): [0] scopes opened, [1] tasks added by
 * check-ins */
void hclib_hip_dyn_finish_stats(uint64_t out[2]);
/* promises [first, first + n) of the last launch: data, and whether put */
int hclib_hip_dyn_datum(uint32_t first, uint32_t n, uint64_t *datum, uint8_t *put);

/* ---------------------------------------------------------------- SW */
typedef struct {
    uint64_t tiles;      /* tile tasks executed */
    uint64_t releases;   /* dependency-counter decrements */
    double kernel_ms;
    double cells_per_s;
    double tile_us;      /* average in-tile DP time per tile task */
    double release_us;   /* average dependency-release time per tile task */
} hclib_hip_sw_result_t;

/* Tiled global alignment of smith_waterman.cpp over host sequences coded
 * 1..4 (A,C,G,T). Tile grid = (n1/tw) x (n2/th); remainders dropped as the
 * reference does. tw must be a multiple of 64... no: any tw <= 4096, th a
 * multiple of 64 or th <= 64*16. Writes the score (bottom-right cell). */
int hclib_hip_sw(const int8_t *s1, size_t n1, const int8_t *s2, size_t n2, int tw, int th,
                 int *score, hclib_hip_sw_result_t *result);

/* The same run, plus a read-back of what every tile put (the reference's
 * three promises per tile, smith_waterman.cpp:212-226), for tests: H values,
 * copied from the device after the run's own synchronise; no kernel differs.
 * The pointers are optional host arrays; `*filled` (may be NULL) receives the
 * HCLIB_HIP_SW_EDGE_* bits of the arrays that were given AND that the
 * schedule that ran keeps on the device:
 *   bottoms [nth][ntw*tw]  H(matrix row (i+1)*th, columns 1..ntw*tw): every
 *                          schedule, except the multi-wave row kernel with
 *                          HCLIB_HIP_SW_ROWS_PER_WG > 1 (a workgroup then
 *                          publishes only its last tile row; bit clear);
 *   rights  [tiles][th]    tile t = i*ntw + j: H(rows i*th+1 .. (i+1)*th,
 *                          column (j+1)*tw): the queue and every promise-DAG
 *                          body. The row schedules keep right columns in LDS
 *                          only: bit clear, array untouched;
 *   corners [tiles]        H((i+1)*th, (j+1)*tw): the tile's own corner word
 *                          (queue, DAG bodies), or the last value of its
 *                          bottom row where the schedule keeps no corner word
 *                          (row schedules; clear when bottoms is).
 * Where the device holds tagged granules, every tag must be set: a granule
 * without its tag is HCLIB_HIP_EDEVICE, the message naming tile and index.
 * `path` / `form` report what ran: HCLIB_HIP_SW_PATH_*, and the multi-wave
 * band form (100 R + 10 S + K / 16, after the fallback for th) or 0. */
#define HCLIB_HIP_SW_EDGE_BOTTOMS 1u
#define HCLIB_HIP_SW_EDGE_RIGHTS 2u
#define HCLIB_HIP_SW_EDGE_CORNERS 4u
#define HCLIB_HIP_SW_PATH_QUEUE 1     /* one wave per tile, dependency counters */
#define HCLIB_HIP_SW_PATH_ROWS1 2     /* row schedule, one wave per tile row */
#define HCLIB_HIP_SW_PATH_BAND_ROWS 3 /* row schedule, multi-wave band rows */
#define HCLIB_HIP_SW_PATH_DAG_WAVE 4  /* promise DAG, one wave per tile */
#define HCLIB_HIP_SW_PATH_DAG_WG 5    /* promise DAG, band workgroup per tile */
#define HCLIB_HIP_SW_PATH_DAG_PK 6    /* promise DAG, packed-half body */
typedef struct {
    int *bottoms;
    int *rights;
    int *corners;
    int path; /* out */
    int form; /* out */
} hclib_hip_sw_edges_t;
int hclib_hip_sw_edges(const int8_t *s1, size_t n1, const int8_t *s2, size_t n2, int tw, int th, int *score,
                       hclib_hip_sw_result_t *result, hclib_hip_sw_edges_t *edges, uint32_t *filled);

/* Column-band session (multi-GPU SW, one band of tile columns per rank).
 * The reference runs the whole tile DAG in one address space
 * (smith_waterman.cpp:168-235); sharded, rank r owns tile columns [j0, j1)
 * and its only inputs from other ranks are the left band's right column
 * (the reference's right_column promises of tile column j0-1, :212-216) and
 * its bottom-right corners (:222-226), both carried by one int array:
 *   begin   uploads s1/s2 (coded 1..4) and allocates the band's granules;
 *   rows    launches tile rows [i0, i1) of the band on `stream` (a
 *           hipStream_t); left_in = device array of nth*th ints holding H of
 *           matrix column j0*tw for rows 1..nth*th (rows up to i1*th must be
 *           in place; NULL only when j0 == 0); right_out (device, nth*th
 *           ints, or NULL) receives H of column j1*tw for the same rows;
 *   end     synchronises the stream, checks the device error word, writes
 *           the band's bottom-right cell (the score for the last band) and
 *           the tiles executed, and frees the band;
 *   bottoms (for tests, before end) synchronises the stream and copies the
 *           band's bottom rows to the host array out[nth][(j1-j0)*tw]: H of
 *           matrix rows (i+1)*th, columns j0*tw+1 .. j1*tw. Every tile row
 *           must have been launched, one tile row per workgroup
 *           (HCLIB_HIP_SW_ROWS_PER_WG unset or 1): a granule without its tag
 *           is HCLIB_HIP_EDEVICE, the message naming tile and index. */
typedef struct hclib_hip_sw_band hclib_hip_sw_band_t;
int hclib_hip_sw_band_begin(const int8_t *s1, size_t n1, const int8_t *s2, size_t n2, int tw, int th,
                            int j0, int j1, hclib_hip_sw_band_t **band);
int hclib_hip_sw_band_rows(hclib_hip_sw_band_t *band, int i0, int i1, const int *left_in, int *right_out,
                           void *stream);
int hclib_hip_sw_band_bottoms(hclib_hip_sw_band_t *band, void *stream, int *out);
int hclib_hip_sw_band_end(hclib_hip_sw_band_t *band, void *stream, int *corner, uint64_t *tiles);

/* ----------------------------------------------------------- Cholesky */
/* The tiled Cholesky factorisation of test/cholesky (cholesky.cpp:80-124 and
 * its four tile kernels) as ONE launch of the device promise DAG: one promise
 * per tile version lkji[j][i][k], one workgroup task per tile kernel, no
 * barrier between the steps. `a` and `l` are host arrays, row-major n x n
 * (`l` may be `a`); only the lower triangle of `a` is read, `l` receives the
 * factor in its lower triangle and +0.0 above it. n % tile == 0 (the
 * reference's own check), tile <= 128.
 *   HCLIB_HIP_CHOL_EXACT  (the one mode) every element sees the reference's
 *       operations in the reference's order (unfused multiply and add,
 *       ascending k, IEEE divide and square root): bit-identical to the
 *       reference for every tile size.
 * A pivot <= 0 is the reference's "Not a symmetric positive definite (SPD)
 * matrix" (sequential_cholesky.cpp:11-12): HCLIB_HIP_EDEVICE, the message
 * holds that text and the column, result->fail_col is set and `l` is not
 * written. Argument errors are HCLIB_HIP_EINVAL before the device is touched. */
#define HCLIB_HIP_CHOL_EXACT 0   /* reference operation order, unfused: bit-identical to test/cholesky */
typedef struct {
    uint64_t tasks, puts, releases;        /* from the DAG launch */
    uint64_t potrf, trsm, syrk, gemm;      /* tasks by kind */
    double kernel_ms;                      /* device events around the one launch */
    double gflops;                         /* (n^3/3) / kernel time */
    int fail_col;                          /* -1, or the global column whose pivot was <= 0 */
} hclib_hip_cholesky_result_t;
int hclib_hip_cholesky(const double *a, int n, int tile, int mode, double *l,
                       hclib_hip_cholesky_result_t *result);

/* --------------------------------------------------------------- sort */
/* BOTS sort (cilksort, test/performance-regression/full-apps/bots/sort:
 * sort.ref.c:315-423, the HClib port sort.c) as ONE launch of dynamic device
 * dataflow: one device task per call of the reference's call tree (four-way
 * sort, binary-split merges), created on the device, its finish scopes as
 * hx::dyn_finish_open / _check_in / _check_out, its leaves wave-wide HIP
 * bodies. `keys` is a host array of n int64, sorted in place. merge_cutoff is
 * the reference's cutoff_value (a merge whose smaller range holds at most
 * that many keys is one task), sort_cutoff its cutoff_value_1 (fewer keys
 * than that are sorted by one task, in LDS: at most 2048); 0 selects the
 * reference's default, 2048. The reference's insertion cutoff has no device
 * meaning. The empty-range copy moves all high1 - low1 + 1 keys (the
 * reference's memcpy, sort.ref.c:344, is one short). The counts are those of
 * the call tree, a function of the input alone. Argument errors are
 * HCLIB_HIP_EINVAL before the device is touched: keys NULL, n < 1 or
 * n >= 2^31, merge_cutoff < 2, sort_cutoff < 4 or > 2048.
 * hclib_hip_sort_bounds: the pool sizes the launch allocates, upper bounds
 * derived from n and the cutoffs for every input: out[0] tasks, out[1]
 * promises (finish scopes), out[2] wait nodes. */
typedef struct {
    uint64_t tasks, sort_leaf, sort_split, merge_leaf, merge_split, merge_empty;
    uint64_t finishes;      /* scopes opened */
    uint64_t check_ins;     /* tasks added by dyn_finish_check_in */
    double kernel_ms;       /* device events around the one launch */
    double keys_per_s;
} hclib_hip_sort_result_t;
int hclib_hip_sort_i64(int64_t *keys, int64_t n, int merge_cutoff, int sort_cutoff,
                       hclib_hip_sort_result_t *result);
int hclib_hip_sort_bounds(int64_t n, int merge_cutoff, int sort_cutoff, uint64_t out[3]);
/* Where the last sort's wave time went: ticks of the 100 MHz device clock
 * summed over the tasks of each class, each from the start of its body to the
 * end of its check-out: [0] sort leaves, [1] sort splits, [2] merge leaves,
 * [3] merge splits, [4] empty-range copies, [5] merge-phase continuations. */
void hclib_hip_sort_last_ticks(uint64_t out[6]);

/* ----------------------------------------------------------- SparseLU */
/* BOTS SparseLU (test/performance-regression/full-apps/bots/sparselu_single,
 * sparselu_for: sparselu.ref.c:300-322, the HClib port sparselu.c) as ONE
 * launch of the device promise DAG. The matrix is S x S blocks of B x B
 * floats; mask[ii * S + jj] != 0 where block (ii, jj) is present. Blocks are
 * block-packed: the present blocks in row-major (ii, jj) order, each B * B
 * floats, row-major. The factorisation has no pivoting and creates blocks
 * (fill-in, sparselu.ref.c:318), so the task graph depends on the mask:
 *
 * hclib_hip_sparselu_genmat  the reference's generator (sparselu.ref.c:86-133):
 *     mask receives S * S bytes, blocks (unless NULL) the present blocks.
 * hclib_hip_sparselu_plan    the symbolic pass, on the host alone: walks the
 *     reference's program order over the mask, marks fill-in and builds the
 *     graph. mask_out (S * S bytes, may be NULL) receives the final structure;
 *     counts (may be NULL): [0] lu0 [1] fwd [2] bdiv [3] bmod tasks, [4] blocks
 *     in, [5] blocks out. payload, await_off and await_ids (all three or none)
 *     receive what hclib_hip_dag_begin takes: 4 words per task {kind (0 lu0,
 *     1 fwd, 2 bdiv, 3 bmod), kk, ii, jj} — the task writes block (ii, jj) —
 *     tasks + 1 await offsets, and at most 3 await ids per task (size them
 *     from a first call's counts). Promise p is put by task p: a task awaits
 *     the last writer of the block it updates and of each block it reads;
 *     blocks nothing has written yet (the upload, a zeroed fill-in) need no
 *     await. An absent diagonal block, S < 1 or more tasks than
 *     hclib_hip_dag_begin accepts (2^32 - 2) are HCLIB_HIP_EINVAL; the tasks
 *     are counted (on row bitsets) before any graph array is built, so the
 *     limit costs no memory. A plan the host cannot hold is HCLIB_HIP_ENOMEM.
 * hclib_hip_sparselu         the factorisation: host arrays in and out;
 *     blocks_out is packed for mask_out ([5] of the plan's counts blocks) and
 *     holds L (unit lower, below the diagonal) and U in place, as the
 *     reference leaves them. Every element sees the reference's operations in
 *     the reference's order (one rounded f32 multiply, one rounded f32
 *     subtract, ascending k, IEEE divide): bit-identical to sparselu_seq_call
 *     for every B. There is no pivot check, as in the reference: a zero pivot
 *     gives inf / NaN and the call still returns HCLIB_HIP_OK. B < 1 or
 *     B > 128 and the plan's errors are HCLIB_HIP_EINVAL before the device is
 *     touched. Packing and both copies are outside kernel_ms.
 *     gflops counts the reference's operations: a divide, and a multiply and
 *     a subtract per update; per task lu0 B(B-1)/2 + (B-1)B(2B-1)/3,
 *     fwd B^2 (B-1), bdiv B^3, bmod 2 B^3.
 * (The calibration of the bmod body alone, hclib_hip_sparselu_bmod_rate, is
 * with the other calibration entries above.) */
typedef struct {
    uint64_t blocks_in, blocks_out;        /* present blocks before and after (fill-in) */
    uint64_t lu0, fwd, bdiv, bmod;         /* tasks by kind */
    uint64_t tasks, puts, releases;        /* from the DAG launch */
    double kernel_ms;                      /* device events around the one launch */
    double gflops;                         /* the reference's operations / kernel time */
    int wgs_per_cu;                        /* persistent workgroups per CU of the launch */
} hclib_hip_sparselu_result_t;
int hclib_hip_sparselu_genmat(int S, int B, uint8_t *mask, float *blocks);
int hclib_hip_sparselu_plan(const uint8_t *mask, int S, uint8_t *mask_out, uint64_t counts[6],
                            uint32_t *payload, uint32_t *await_off, uint32_t *await_ids);
int hclib_hip_sparselu(const uint8_t *mask, const float *blocks, int S, int B,
                       uint8_t *mask_out, float *blocks_out, hclib_hip_sparselu_result_t *result);

/* ------------------------------------------------------------ N-Queens */
/* N-Queens on the persistent work-stealing scheduler (the one fib and UTS run
 * on), in the reference's two forms:
 *   HCLIB_HIP_NQUEENS_BOTS  test/performance-regression/full-apps/bots/nqueens/
 *       nqueens.c:125-182: every call nqueens(n, j, a) with j < n opens a finish
 *       scope and spawns its column tasks; the counts are summed up the scopes
 *       (`*solutions += csols[i]`), the root scope's value is the answer.
 *   HCLIB_HIP_NQUEENS_FLAT  test/performance-regression/full-apps/nqueens.cpp:
 *       41-60 (and test/misc/nqueens.cpp): one outer finish, an async only for a
 *       placement that passes ok(), one counter (here: one per lane, summed).
 * task_depth is the BOTS manual cutoff: a call with j >= task_depth is finished
 * by one lane's serial search (nqueens_ser); 0, or anything >= n, means every
 * call spawns, as both HClib ports do.
 * result->solutions is the count. tasks and scopes are the reference's: with
 * P(n, j) = the valid prefixes of j queens and m = the effective task depth,
 * BOTS scopes = the sum of P(n, j) over j < m (one finish per spawning call) and
 * tasks = n * scopes (its n asyncs); flat tasks = the sum of P(n, j) over
 * 1 <= j <= m, scopes = 0. items is what the device ran: in the BOTS form the
 * parent settles a conflicting placement itself (the scope counts the free
 * columns only, and a call with no free column closes at once on a sum of zero
 * without a scope of its own), so items is far below tasks; both include the
 * root item, which stands for the call nqueens(n, 0). joins = scopes closed.
 * hist (n + 1 entries, or NULL): hist[j] = P(n, j), counted by the tasks and by
 * the lanes' serial searches alike (a separate kernel instantiation).
 * HCLIB_HIP_EINVAL before the device is touched: n < 1 or n > 20, a form that
 * is neither of the two, task_depth < 0, result NULL, and in the BOTS form a
 * scope count above what the arena can address (0xfffffff0 less the 2^24 ids
 * reserved for the workers' id blocks). The BOTS arena holds every scope once;
 * its exact size is a depth-first search on the host, outside kernel_ms.
 * hclib_hip_nqueens_bounds: host only, no GPU: out[0] tasks, out[1] scopes as
 * above for (n, form, task_depth), with the same argument checks (in the flat
 * form the count walks every prefix up to the task depth: the whole search
 * when every call spawns). */
typedef struct {
    uint64_t solutions, tasks, items, scopes, joins, chunks_pushed, chunks_stolen;
    double kernel_ms, busy_frac;
} hclib_hip_nqueens_result_t;
#define HCLIB_HIP_NQUEENS_BOTS 0
#define HCLIB_HIP_NQUEENS_FLAT 1
int hclib_hip_nqueens(int n, int form, int task_depth, hclib_hip_nqueens_result_t *result,
                      uint64_t *hist /* n + 1 entries, may be NULL */);
int hclib_hip_nqueens_bounds(int n, int form, int task_depth, uint64_t out[2]);

/* ------------------------------------------------------------ Strassen */
/* BOTS Strassen (test/performance-regression/full-apps/bots/strassen:
 * strassen.ref.c the algorithm, strassen.c the HClib port) as ONE launch of
 * dynamic device dataflow: C = A x B by OptimizedStrassenMultiply(C, A, B, n,
 * n, n, n), every call of its tree a device task, the port's finish scopes as
 * dyn_finish_*, the two sweeps of a call split into bands of band_rows rows
 * that check in to a scope dynamically (hclib_amd/csrc/strassen.hip has the
 * task graph). a, b, c are host arrays of n x n doubles, row-major and dense.
 * cutoff is the reference's (a product of at most cutoff rows is multiplied
 * directly); 0 selects its default, 64. band_rows 0 selects 8, or 16 where
 * the tree has 8192 or more leaf multiplies (bases, or the 64 x 64 tiles of
 * larger bases): n >= 2048 at the default cutoff.
 * The result is bit-identical to OptimizedStrassenMultiply_seq compiled
 * without fused multiply-add: the reference's operation order in both sweeps,
 * and in a base product, for every element, the chain over ascending k that
 * starts from the first product (not from 0.0), each product and each sum
 * rounded on its own. (The reference's driver passes its matrices in another
 * order than strassen_main_par declares them and checks two matrices nobody
 * wrote; the target here is the multiply itself)
 * HCLIB_HIP_EINVAL before the device is touched: a, b or c NULL, n not a
 * power of two, n < 16, n > 16384, cutoff in 1 .. 15 (or negative: the
 * reference's naive kernels step 8 columns on a quadrant of 8 x 8 at the
 * least), band_rows < 0, and a call tree whose arena (3 n^2 doubles and the
 * temporaries) reaches 2^32 doubles, which the tasks' 32-bit element offsets
 * cannot address. An arena the device cannot hold is HCLIB_HIP_ENOMEM.
 * tasks .. check_ins are what the device ran and equal the bounds; base counts
 * the products of at most cutoff rows, tiles the 64 x 64 tile tasks of bases
 * larger than 64. workspace_bytes is the temporaries: eleven quadrants per
 * splitting call, all calls live at once (258 MB at n = 1024 / cutoff 64); the
 * three matrices sit in front of them. Both copies are outside kernel_ms.
 * hclib_hip_strassen_bounds: host only, no GPU: out[0] tasks, out[1] finish
 * scopes (promises), out[2] wait nodes, out[3] workspace bytes, all exact (the
 * tree does not depend on the data); the launch allocates exactly these. The
 * same argument checks, but for the matrices.
 * hclib_hip_strassen_last_ticks: where the last launch's wave time went, ticks
 * of the 100 MHz device clock summed over the tasks of each class, each from
 * the start of its body to the end of its check-out: [0] base and tile
 * multiplies, [1] PRE bands, [2] COMBINE bands, [3] MUL splits, [4] FORK,
 * [5] POST. */
typedef struct {
    uint64_t tasks, splits, base, tiles, pre_bands, combine_bands;
    uint64_t finishes, check_ins;
    uint64_t workspace_bytes;
    double kernel_ms;     /* device events around the one launch */
    double gflops;        /* 2 n^3 / kernel time: the classical count, not what Strassen executes */
} hclib_hip_strassen_result_t;
int hclib_hip_strassen(const double *a, const double *b, double *c, int n,
                       int cutoff, int band_rows, hclib_hip_strassen_result_t *result);
int hclib_hip_strassen_bounds(int n, int cutoff, int band_rows, uint64_t out[4]);
void hclib_hip_strassen_last_ticks(uint64_t out[6]);

/* -------------------------------------------------------------- Health */
/* BOTS Health (test/performance-regression/full-apps/bots/health: health.ref.c
 * the algorithm, health.c the HClib port) as ONE launch of dynamic device
 * dataflow: sim_time rounds of sim_village_par over a tree of `level` levels
 * with `cities` children per village. Every village is a task per round; one
 * with children opens a finish scope for them, works on its own hospital while
 * they run, and a continuation behind the scope takes in the patients they
 * sent up, smallest id first (hclib_amd/csrc/health.hip has the task graph and
 * the layout). The lists are arrays of patient ids, walked 64 at a time.
 * params are the ten settings of a BOTS input file, in the file's order; seed
 * is the low 32 bits of what the reference reads with %ld.
 * The full final state is bit-identical to the reference's (any schedule, any
 * compiler: every draw comes from the patient's own seed, and the reallocated
 * patients are taken by id): my_rand on wrapping 32-bit words, its value one
 * int -> float conversion and one f32 multiply by 2^-31.
 * result: the nine sums of get_results (:197-276), sums of integers (the
 * reference adds each time and each visit count as a float to a long: the same
 * number while a sum is below 2^24); tasks, finishes and check_ins are what the
 * device ran and equal the bounds: check_ins counts the tasks checked in to
 * scopes, cities + 1 at every open. leaf_calls, inner_calls and posts are the
 * tasks by class. rounds_per_s = sim_time / kernel time; the upload of the
 * initial state and the download are outside kernel_ms.
 * state (may be NULL) receives the final state into the caller's arrays:
 * seed, time, time_left and hosps_visited, one word per patient, indexed by
 * patient id (the reference's sim_pid order); village, seven words per village
 * in the reference's allocation order (a village, then its children cities ..
 * 1 with their subtrees): id, level, free_personnel, |population|, |waiting|,
 * |assess|, |inside|; lists, one id per patient: village by village the four
 * lists in that order, each in list order. Size them from the bounds.
 * HCLIB_HIP_EINVAL before the device is touched: params or result NULL, a NULL
 * array in state; level, cities or population_ratio < 1, sim_time < 0;
 * assess_time or convalescence_time < 1 (a zero makes time_left step past zero
 * and never return); a probability outside [0, 1] or NaN; cities * 2^(level-1)
 * above 2048 (the most patients one village can receive in a round, which it
 * sorts in LDS); level > 24, 2^31 or more villages or patients, 2^32 or more
 * list words, or 2^32 - 16 or more tasks (sim_time * (villages + villages with
 * children)), which 32-bit indices cannot address. sim_time = 0 is valid and
 * returns the initial state without a launch. An arena the device cannot hold
 * is HCLIB_HIP_ENOMEM.
 * hclib_hip_health_bounds: host only, no GPU: out[0] villages, out[1]
 * patients, out[2] tasks, out[3] finish scopes (promises), out[4] wait nodes,
 * out[5] bytes of the arena (class counters, village tables, records, lists),
 * all exact closed forms; the launch allocates exactly these. The same
 * argument checks.
 * hclib_hip_health_last_ticks: where the last launch's wave time went, ticks
 * of the 100 MHz device clock summed over the tasks of each class, check-out
 * included: [0] CALL of a village without children, [1] CALL of one with
 * children, [2] POST. */
typedef struct {
    int level, cities, population_ratio, sim_time, assess_time, convalescence_time;
    int32_t seed;
    float get_sick_p, convalescence_p, realloc_p;
} hclib_hip_health_params_t;
typedef struct {
    int64_t population, hospitals, personnel, hosps_visited, in_village, waiting, assess, inside, total_time;
    uint64_t tasks, finishes, check_ins;
    uint64_t leaf_calls, inner_calls, posts;
    double kernel_ms;     /* device events around the one launch */
    double rounds_per_s;
} hclib_hip_health_result_t;
typedef struct {
    int32_t *seed, *time, *time_left, *hosps_visited; /* patients words each */
    int32_t *village;                                 /* villages x 7 */
    int32_t *lists;                                   /* patients words */
} hclib_hip_health_state_t;
int hclib_hip_health(const hclib_hip_health_params_t *params, hclib_hip_health_result_t *result,
                     hclib_hip_health_state_t *state /* may be NULL */);
int hclib_hip_health_bounds(const hclib_hip_health_params_t *params, uint64_t out[6]);
void hclib_hip_health_last_ticks(uint64_t out[3]);

/* ------------------------------------------------------------ Floorplan */
/* BOTS floorplan (test/performance-regression/full-apps/bots/floorplan:
 * floorplan.c:230-328, the algorithm in floorplan.ref.c) on the persistent
 * work-stealing scheduler: a branch-and-bound search for the smallest bounding
 * box of n cells on a 64 x 64 board. Each cell has up to 8 shapes and is placed
 * against its `left` and / or `above` cell (0: the dummy cell, which puts cell
 * 1 in column 0; -1: none), in the order 1, next[1], ... One task per (shape,
 * north-west corner) candidate, in the reference's order; a candidate that is
 * not the last cell spawns the next cell's candidates iff its area is below
 * the bound, one word that complete placements lower while the search runs.
 * The input's arrays are indexed by cell id 1..n (entry 0 is ignored).
 * flags: HCLIB_HIP_FLOORPLAN_NOPRUNE compares against the constant 4096
 * instead (the bound is still tracked): the search is exhaustive and every
 * count is the same on every run. Pruned, min_area and its footprint are
 * deterministic; the counts and, among placements of equal area, the one
 * returned depend on the schedule, as in the reference.
 * result: min_area (4096 and a 0 x 0 footprint when no complete placement
 * exists, as the reference prints), footprint = {rows, columns}, placements
 * [id - 1] = the shape index and north-west corner of cell id (-1s without a
 * placement). tasks = the candidates spawned (bots_number_of_tasks), items =
 * what the device ran (every candidate is one item: items == tasks), laid =
 * candidates that were laid down, complete = complete placements reached,
 * improvements = successful lowerings of the bound.
 * board (4096 bytes, or NULL): the best board, row-major, cell ids, 0 empty.
 * hist (n + 1 entries, or NULL): hist[d] = candidates of the d-th cell of the
 * chain that were laid down (hist[0] = 0); a separate kernel instantiation.
 * A rectangle that leaves the board does not fit (the reference indexes past
 * its board there).
 * HCLIB_HIP_EINVAL before the device is touched: n < 1 or n > 20; a cell with
 * fewer than 1 or more than 8 shapes; a shape dimension outside 1..64; left,
 * above or next outside the table; a cell with neither left nor above, or one
 * that depends on a cell the chain places later (the reference reads
 * rectangles that do not exist); a next chain from cell 1 that does not visit
 * every cell exactly once before 0; result NULL; an unknown flag.
 * hclib_hip_floorplan_read_input: host only, no GPU: the reference's file
 * format (read_inputs, floorplan.c:159-195) with the optional trailing
 * expected minimum area (solution, -1 without one), checked as above. */
#define HCLIB_HIP_FLOORPLAN_MAX_CELLS 20
#define HCLIB_HIP_FLOORPLAN_MAX_SHAPES 8
#define HCLIB_HIP_FLOORPLAN_NOPRUNE 1
typedef struct {
    int32_t n;
    int32_t solution; /* the file's expected minimum area, or -1 */
    int32_t shapes[HCLIB_HIP_FLOORPLAN_MAX_CELLS + 1];
    int32_t shape[HCLIB_HIP_FLOORPLAN_MAX_CELLS + 1][HCLIB_HIP_FLOORPLAN_MAX_SHAPES][2]; /* rows, columns */
    int32_t left[HCLIB_HIP_FLOORPLAN_MAX_CELLS + 1];
    int32_t above[HCLIB_HIP_FLOORPLAN_MAX_CELLS + 1];
    int32_t next[HCLIB_HIP_FLOORPLAN_MAX_CELLS + 1];
} hclib_hip_floorplan_input_t;
typedef struct {
    int32_t shape, top, lhs;
} hclib_hip_floorplan_placement_t;
typedef struct {
    int32_t min_area;
    int32_t footprint[2];
    hclib_hip_floorplan_placement_t placements[HCLIB_HIP_FLOORPLAN_MAX_CELLS];
    uint64_t tasks, items, laid, complete, improvements, chunks_pushed, chunks_stolen;
    double kernel_ms, busy_frac;
} hclib_hip_floorplan_result_t;
int hclib_hip_floorplan(const hclib_hip_floorplan_input_t *in, int flags, hclib_hip_floorplan_result_t *result,
                        uint8_t *board /* 4096, may be NULL */, uint64_t *hist /* n + 1, may be NULL */);
int hclib_hip_floorplan_read_input(const char *path, hclib_hip_floorplan_input_t *out);

/* ------------------------------------------------------------ Alignment */
/* BOTS alignment (test/performance-regression/full-apps/bots/alignment_for and
 * alignment_single: alignment.ref.c the algorithm, alignment.c the HClib port,
 * one hclib_async per sequence pair inside one hclib_start_finish; the two
 * programs differ only in the host loop that creates those tasks) as ONE
 * launch of dynamic device dataflow: every pair si < sj of the input aligned
 * by forward_pass, reverse_pass and Myers-Miller's diff with affine gaps, the
 * protein branch, and scored by the percentage of identical residues on the
 * alignment's diagonal steps. A task per pair runs the two passes and the root
 * diff; a diff of more than `cutoff` cells (M * N) computes its midpoint and
 * creates its two halves as tasks, a smaller one runs the whole recursion below
 * it from a stack in LDS. Every task body is wave-wide and is the serial
 * recurrence itself (hclib_amd/csrc/alignment.hip has the sweep). Integers
 * only on the device; the gap-open penalty (a log) and the final percentage
 * are computed on the host in double as the reference computes them, so every
 * score and every field of a pair's record equals the reference's on any
 * schedule and at any cutoff.
 * input: nseqs sequences of residue codes 0..24 by "ABCDEFGHIKLMNPQRSTUVWXYZ-",
 * a '-' of the file as 31; sequence i is codes[offset[i] .. offset[i] +
 * length[i]). names (may be NULL) has 31 bytes per sequence.
 * matrix: mat_avscore and matrix[32][32] as the reference's get_matrix leaves
 * them; the library carries no substitution table of its own.
 * cutoff: cells, at least 1; 0 chooses the default 16384.
 * result: scores, the caller's nseqs x nseqs ints, receives bench_output (the
 * upper triangle, zeros elsewhere, 1 for a pair with an empty sequence). pairs
 * = the pairs without an empty sequence, each a pair task. tasks = what the
 * device ran = 1 + pairs + 2 x (diffs that created their halves); created = the
 * tasks device tasks created (tasks - 1); promises = 0. pair_tasks, spawn_tasks
 * and leaf_tasks count the tasks by class: pairs, diff tasks that created their
 * halves, diff tasks that did not. matches, diff_calls, type2 and ties are the
 * sums of the records. cells = the sum of n * m over the pairs; cells_per_s =
 * cells / kernel time; uploads and the download are outside kernel_ms.
 * pairs (may be NULL; `pairs` entries, hclib_hip_alignment_bounds out[0]), in
 * (si, sj) order: si, sj (from 0), g, gh, what the passes found (maxscore, se1,
 * se2, sb1, sb2, positions from 1), and over the pair's diff tree: matches
 * (diagonal steps with equal residues that are no gap codes), diff_calls (every
 * invocation, base cases included), type2 (midpoints of type 2) and ties (takes
 * of the midpoint scan's hh == midh && HH[j] != DD[j] && RR[j] == SS[j]
 * branch).
 * HCLIB_HIP_EINVAL before the device is touched: a NULL input, matrix, result
 * or result->scores; nseqs < 1; a length below 0 or above 4999 (the
 * reference's MAX_ALN_LENGTH arrays hold no more, and it would overflow them
 * silently); a sequence outside codes; a code above 31; cutoff < 0; a matrix
 * whose avscore makes a gap penalty negative.
 * hclib_hip_alignment_read_input: host only, no GPU: a Pearson file with the
 * reference's behaviour (readseqs, sequence.c:120-186): the `Number of
 * sequences is <n>` line, names up to the first blank, only the 24 upper-case
 * letters of the code string and '-' kept (the reference's table maps a
 * lower-case letter to its upper-case one and then rejects it by comparison),
 * an empty sequence legal when a line follows its header. EINVAL for a file the
 * reference would read out of bounds on: no count line, fewer sequences than
 * the count, a last header with nothing after it, a sequence over 4999. The
 * arrays are the library's; give them back with _free_input.
 * hclib_hip_alignment_read_matrix: host only: a matrix file, '#' comment lines,
 * `avscore <int>`, then 32 x 32 integers.
 * hclib_hip_alignment_bounds: host only: out[0] pairs (exact), and upper bounds
 * in closed form on what a launch at this cutoff uses: out[1] tasks, out[2]
 * diffs that create their halves, out[3] diff calls, out[4] bytes of the arena
 * with the most resident waves a launch can have, out[5] bytes of one wave's
 * row arrays in it (0: they are in LDS, the longest sequence has at most 767
 * residues). The pools of a launch are sized from these. The same checks.
 * hclib_hip_alignment_last_ticks: where the last launch's wave time went, ticks
 * of the 100 MHz device clock summed over the tasks of each class: [0] the
 * root, [1] pair tasks, [2] diff tasks that created their halves, [3] diff
 * tasks that did not. */
typedef struct {
    int32_t nseqs, total; /* total: entries of codes */
    int32_t *length;      /* nseqs */
    int32_t *offset;      /* nseqs */
    uint8_t *codes;       /* total */
    char *names;          /* nseqs x 31, or NULL */
} hclib_hip_alignment_input_t;
typedef struct {
    int32_t avscore;
    int32_t score[32][32];
} hclib_hip_alignment_matrix_t;
typedef struct {
    int32_t si, sj, g, gh, maxscore, se1, se2, sb1, sb2, matches, diff_calls, type2, ties;
} hclib_hip_alignment_pair_t;
typedef struct {
    int32_t *scores; /* nseqs x nseqs, the caller's */
    uint64_t pairs, tasks, created, promises, pair_tasks, spawn_tasks, leaf_tasks;
    uint64_t matches, diff_calls, type2, ties, cells;
    int32_t cutoff; /* the cutoff used */
    double kernel_ms; /* device events around the one launch */
    double cells_per_s;
} hclib_hip_alignment_result_t;
int hclib_hip_alignment(const hclib_hip_alignment_input_t *input, const hclib_hip_alignment_matrix_t *matrix, int cutoff,
                        hclib_hip_alignment_result_t *result, hclib_hip_alignment_pair_t *pairs /* may be NULL */);
int hclib_hip_alignment_read_input(const char *path, hclib_hip_alignment_input_t *out);
void hclib_hip_alignment_free_input(hclib_hip_alignment_input_t *in);
int hclib_hip_alignment_read_matrix(const char *path, hclib_hip_alignment_matrix_t *out);
int hclib_hip_alignment_bounds(const hclib_hip_alignment_input_t *input, int cutoff, uint64_t out[6]);
void hclib_hip_alignment_last_ticks(uint64_t out[4]);

/* BOTS fft (test/performance-regression/full-apps/bots/fft: fft.ref.c the
 * algorithm, fft.c the HClib port): the Cilk mixed-radix transform fft_seq(n,
 * in, out) as ONE launch of dynamic device dataflow, every output bit-identical
 * to the reference's given the reference's twiddle table. A call above the
 * cutoff is a task that opens a finish scope for the bands of its unshuffle, a
 * continuation that opens one for its r children (the two buffers' roles
 * swapped), and a continuation that runs the twiddle sweep as bands
 * (hclib_amd/csrc/fft.hip has the task table); a call of at most `cutoff`
 * points, and every base of 2 .. 32 points, is one task that runs its whole
 * subtree pass by pass. Radix-2 / 4 / 8 / 16 columns are butterflies in a
 * lane's registers, f64 VALU without fused multiply-add.
 * `in` and `out` are n interleaved (re, im) pairs of the host; `in` is not
 * written. `w` is the table W of n + 1 (re, im) pairs the transform reads, an
 * input: the reference's binary computes it with a libm call whose last bit no
 * formula restates, so a caller that wants the reference's bits passes the
 * reference's table. NULL: hclib_hip_fft_twiddles(n), the reference's formula
 * and write order through this host's cos and sin.
 * cutoff: 0 (8192) or at least 32. band: columns (for the general radix,
 * outputs) per band task, 0 (256, or 1024 for n above 2^22) or a multiple of
 * 64. Results depend on neither. The launch reads HCLIB_HIP_FFT_WAVES_PER_CU
 * (1, or 4 for n above 2^22; at most 8). EINVAL unless 1 <= n <= 2^26 and n's largest prime factor is at most
 * 512; ENOMEM where the device cannot hold 3 x 16 n bytes.
 * hclib_hip_fft_factors: host only: fft_seq's factor list, its length returned
 * (negative: EINVAL). Calls of 2 .. 32 points are bases whatever the list says.
 * hclib_hip_fft_twiddles: host only: n + 1 pairs into w.
 * hclib_hip_fft_bounds: host only, exact: out[0] tasks, out[1] finish scopes,
 * out[2] wait nodes, out[3] leaf tasks, out[4] band tasks, out[5] bytes the
 * passes move (32 n per pass: every pass reads and writes each pair once).
 * hclib_hip_fft_last_ticks: where the last launch's wave time went, ticks of
 * the 100 MHz device clock summed over the tasks of each class: [0] leaves,
 * [1] UNSH bands, [2] TWID bands, [3] CALL, [4] FORK, [5] POST. */
typedef struct {
    uint64_t tasks, leaves, calls, unsh_bands, twid_bands;
    uint64_t finishes, check_ins;
    uint64_t bytes_moved;      /* out[5] of _bounds */
    int32_t nfactors, factors[40];
    int32_t cutoff, band;      /* the values used */
    double kernel_ms;          /* device events around the one launch */
    double gbytes_per_s;       /* bytes_moved / kernel_ms */
} hclib_hip_fft_result_t;
int hclib_hip_fft(const double *in, double *out, int n, const double *w /* n + 1 pairs, or NULL */, int cutoff, int band,
                  hclib_hip_fft_result_t *result);
int hclib_hip_fft_factors(int n, int out[40]);
int hclib_hip_fft_twiddles(int n, double *w);
int hclib_hip_fft_bounds(int n, int cutoff, int band, uint64_t out[6]);
void hclib_hip_fft_last_ticks(uint64_t out[6]);

/* Kastors Jacobi (test/performance-regression/full-apps/kastors-1.1/jacobi:
 * jacobi-seq.c the rule, jacobi-task.c, jacobi-block-task.c and
 * jacobi-block-for.c its three parallel sweeps, poisson.c the driver): niter
 * sweeps of the 5-point stencil over a row-major nx x ny grid of doubles,
 * a[i * ny + j], as ONE launch of the device promise DAG with no barrier
 * between sweeps. Per sweep a boundary cell becomes f, every other cell
 * 0.25 * ((((u[i-1][j] + u[i][j+1]) + u[i][j-1]) + u[i+1][j]) + (f[i][j] * dx) * dy)
 * of the sweep before, every operation rounded on its own: the bits of
 * sweep_seq and of the three parallel forms.
 * A task advances one block x block tile by up to `fuse` sweeps from LDS: it
 * reads a halo `fuse` cells wide and recomputes the overlap, which divides the
 * memory traffic and the task count by nearly `fuse` and changes no bit
 * (hclib_amd/csrc/hx_jacobi_plan.h has the graph, jacobi.hip the body).
 * f, unew0 (the initial estimate, poisson.c's unew before sweep()) and unew are
 * host arrays of nx * ny doubles; f and unew0 are not written. niter = 0
 * launches nothing and copies unew0.
 * block: 0 = 128 (run()'s default), else it must divide nx and ny. fuse: 0 =
 * the default (4, or what the block allows), else 1 <= fuse <= block. EINVAL,
 * before the device is touched, unless nx, ny >= 3, niter >= 0, the block
 * divides both sides, block + 2 * fuse <= 82 (three images of a task's region
 * in the CU's LDS; the reference's default block of 128 does not fit, so a
 * caller names a smaller one) and the launch has fewer than 2^26 tasks. Results depend on neither block
 * nor fuse. The launch reads HCLIB_HIP_JACOBI_WGS_PER_CU (default and at most:
 * what the region's LDS allows, 1, 2 or 4).
 * hclib_hip_jacobi_rhs: host only: rhs() and run()'s initial estimate through
 * the host's libm (either array may be NULL).
 * hclib_hip_jacobi_bounds: host only, exact: out[0] tasks, out[1] awaits,
 * out[2] supersteps, out[3] bytes moved (per task the clipped region of u it
 * reads, the cells of f its sweeps read and the block it writes, times 8);
 * EINVAL as the launch would. */
typedef struct {
    uint64_t tasks, puts, releases;      /* from the DAG launch */
    uint64_t supersteps, bytes_moved;    /* the plan's */
    int block, fuse, wgs_per_cu;         /* as run */
    double kernel_ms;                    /* device events around the one launch */
    double gbytes_per_s, gcells_per_s;   /* bytes_moved, and nx*ny*niter, over kernel time */
} hclib_hip_jacobi_result_t;
int hclib_hip_jacobi(const double *f, const double *unew0, int nx, int ny, double dx, double dy,
                     int block, int niter, int fuse, double *unew, hclib_hip_jacobi_result_t *result);
int hclib_hip_jacobi_rhs(int nx, int ny, double *f, double *unew0);
int hclib_hip_jacobi_bounds(int nx, int ny, int block, int niter, int fuse, uint64_t out[4]);

/* Rodinia BFS (test/performance-regression/full-apps/rodinia/bfs/bfs.cpp; the
 * algorithm as bfs.ref.cpp:135-183 states it): the hop count of every vertex
 * from `source` over a directed graph in Rodinia's layout, vertex v owning
 * edges[starting[v] .. starting[v] + degree[v]) (Node::starting and
 * Node::no_of_edges, :32-36), as ONE launch of the work-stealing megakernel.
 * cost[v] is the reference's h_cost: -1 where v is not reached (:128-131).
 *   HCLIB_HIP_BFS_LEVEL  the reference's schedule, level by level (the do /
 *       while of :139-182 with its two sweeps and the wait after each), made
 *       work-efficient: a level is a range of `order`, the vertices in the
 *       order they were claimed (h_graph_visited and h_updating_graph_mask in
 *       one), a vertex of the level is an item whose children are its edges,
 *       an edge claims its head with one compare-and-swap on cost. No wave
 *       waits for a level to end: every wave counts the items it ran, and the
 *       wave whose count completes the level opens the next (the scheduler's
 *       renew hook, include/hclib_hip/hx_sched.h).
 *   HCLIB_HIP_BFS_ASYNC  no levels: an edge lowers cost[head] with an atomic
 *       minimum and a strict lowering makes head's edges items again; an item
 *       whose vertex has since got a lower cost does nothing. The same cost
 *       array bit for bit, at the price of the edges relaxed more than once.
 * result: levels = the reference's sweep count k (:180), the eccentricity of
 * the source + 1; reached = vertices with cost >= 0; relaxed = edge items that
 * ran their atomic (level form: the degrees of the reached vertices summed);
 * items = every item run (level form: reached + relaxed; async form: 1 +
 * relaxed + the edge items that found their vertex out of date).
 * frontier (may be NULL): n_nodes words, frontier[L] = vertices at cost L, 0
 * from `levels` on. order (may be NULL, level form only): n_nodes words, the
 * reached vertices level after level, within a level in claiming order (which
 * differs from run to run), the rest -1.
 * EINVAL, before the device is touched, where the reference's behaviour is
 * undefined: a NULL array (edges may be NULL when n_edges is 0), n_nodes < 1
 * or >= 2^24, n_edges < 0, source outside [0, n_nodes), a degree < 0 or
 * >= 2^24, starting[v] < 0 or starting[v] + degree[v] > n_edges, an edge head
 * outside [0, n_nodes), an unknown form, order with the async form.
 * The launch reads HCLIB_HIP_BFS_CHUNK (items per stolen chunk, 32) and the
 * scheduler's HCLIB_HIP_BFS_SPILL_HI / _SPILL_LO / _HUNGER.
 * hclib_hip_bfs_bounds: host only, with the same checks: out[0] = the bytes of
 * device memory the form takes, out[1] = n_nodes + n_edges, which no launch's
 * level-form item count exceeds.
 * hclib_hip_bfs_read_input: host only: Rodinia's text format read as the
 * reference's fscanf sequence reads it (:84-121): the node count, a (start,
 * degree) pair per node, the source, the edge count, an (id, weight) pair per
 * edge with the weight dropped. With every array NULL it only sizes: counts[0]
 * = nodes, counts[1] = edges, counts[2] = source. Otherwise the arrays have
 * the sizes a first call reported (EINVAL if the file's counts differ). */
typedef struct {
    uint64_t levels, reached, relaxed, items, chunks_pushed, chunks_stolen;
    double kernel_ms, busy_frac;
} hclib_hip_bfs_result_t;
#define HCLIB_HIP_BFS_LEVEL 0
#define HCLIB_HIP_BFS_ASYNC 1
int hclib_hip_bfs(const int32_t *starting, const int32_t *degree, int n_nodes, const int32_t *edges, int n_edges,
                  int source, int form, int32_t *cost, hclib_hip_bfs_result_t *result,
                  uint64_t *frontier /* n_nodes entries, may be NULL */,
                  int32_t *order /* n_nodes entries, may be NULL; level form */);
int hclib_hip_bfs_bounds(const int32_t *starting, const int32_t *degree, int n_nodes, const int32_t *edges,
                         int n_edges, int source, int form, uint64_t out[2]);
int hclib_hip_bfs_read_input(const char *path, int32_t *starting, int32_t *degree, int32_t *edges, int64_t counts[3]);

/* Rodinia CFD (test/performance-regression/full-apps/rodinia/cfd/
 * euler3d_cpu_double.cpp; the arithmetic as euler3d_cpu_double.ref.cpp states
 * it): `iterations` iterations of the three-stage Runge-Kutta Euler solver over
 * an unstructured mesh, as ONE launch of the device promise DAG, bit-identical
 * to the reference built without fused multiply-add.
 * The mesh is what the reference holds after reading (:417-455): nelr = 8 *
 * ceil(nel / 8) rows, the rows from nel on copies of row nel - 1; areas[nelr];
 * neighbours[nelr * 4], an element index >= 0, -1 a wing face, -2 a far-field
 * face (any other negative: a face without a flux, as the reference's chain of
 * ifs leaves it); normals[nelr * 4 * 3], already negated.
 * variables0: nelr * 5 doubles (density, momentum x y z, density energy per
 * element), or NULL for the far field everywhere (:127-130, :383-408).
 * variables: nelr * 5 doubles, the state after the last iteration (dump()
 * prints its first nel rows). iterations == 0 launches nothing and copies the
 * initial state.
 * block: elements per task, a multiple of 8 in [8, 1024], 0 = 256. The result
 * does not depend on it.
 *   HCLIB_HIP_CFD_DAG     one task per (stage, block), stage = 3 iteration + j;
 *       a task awaits, of the stage before, the blocks its elements' faces
 *       name, the blocks that name it, and itself (hclib_amd/csrc/
 *       hx_cfd_plan.h has why this orders the two state buffers' overwrites).
 *   HCLIB_HIP_CFD_PHASES  the same element body as one plain kernel per stage,
 *       stream-ordered: the reference's join per sweep, for comparison.
 * result: tasks, puts, releases from the DAG launch (phases: tasks = the
 * workgroups run, no puts); stages = 3 iterations; bytes_moved = the plan's
 * traffic model; kernel_ms; elements_per_s = nelr * stages over kernel time.
 * EINVAL, before the device is touched, where the reference reads outside its
 * arrays: a NULL array, nel < 1 (or so large that the reference's int indices
 * overflow), iterations < 0, an unknown form, a block outside its limits, a
 * neighbour index >= nelr (one in [nel, nelr) names a padded copy and is
 * accepted), 3 * iterations * nblocks >= 2^26 tasks or 2^32 awaits.
 * hclib_hip_cfd_bounds: host only, with the same checks, exact: out[0] tasks,
 * [1] awaits, [2] stages, [3] the longest waiter list of a promise, [4] the
 * bytes of device memory, [5] bytes_moved.
 * hclib_hip_cfd_read_input: host only: the reference's reader. With every
 * array NULL it only sizes: counts[0] = nel, counts[1] = nelr. Otherwise the
 * arrays hold nelr rows and counts[0] is the nel a first call reported. EINVAL
 * for a file that cannot be opened, is truncated or holds a token that is no
 * number, and for nel < 1. */
typedef struct {
    uint64_t tasks, puts, releases;   /* from the DAG launch */
    uint64_t stages, bytes_moved;     /* the plan's */
    int block, form;                  /* as run */
    double kernel_ms;                 /* device events around the launch (phases: around all stages) */
    double elements_per_s;            /* nelr * stages over kernel time */
} hclib_hip_cfd_result_t;
#define HCLIB_HIP_CFD_DAG 0
#define HCLIB_HIP_CFD_PHASES 1
int hclib_hip_cfd(int nel, const double *areas, const int *neighbours, const double *normals,
                  const double *variables0 /* NULL: far field */, int iterations, int block, int form,
                  double *variables /* nelr * 5 */, hclib_hip_cfd_result_t *result);
int hclib_hip_cfd_read_input(const char *path, double *areas, int *neighbours, double *normals, int64_t counts[2]);
int hclib_hip_cfd_bounds(int nel, const int *neighbours, int iterations, int block, uint64_t out[6]);

/* Rodinia SRAD, speckle-reducing anisotropic diffusion (test/performance-
 * regression/full-apps/rodinia/srad/srad.cpp; the arithmetic as srad.ref.cpp
 * states it): `niter` iterations over a rows x cols float image as ONE launch
 * of the device promise DAG, bit-identical to the reference built without fused
 * multiply-add (its mixed float / double expressions kept operation by
 * operation) wherever the reference's result holds no NaN (a NaN arises only
 * from 0/0, a flat cell inside a zero-variance region; its bits differ between
 * processors).
 * j0: rows * cols floats, row-major, the image after the reference's
 * `J = (float)exp(I)` (hclib_hip_srad_image makes the reference's own).
 * r1..r2, c1..c2: the region of interest, rows and columns, both ends included.
 * lambda: the update's weight. j: rows * cols floats, the image after the last
 * iteration; niter == 0 launches nothing and copies j0. q0sqr: niter floats or
 * NULL: each iteration's scalar of the serial section (srad.ref.cpp:131-141),
 * read back from the reduce promises' datums.
 * block: the side of a task's square block, 16, 32 or 64, dividing both sides;
 * 0 = the largest of 64, 32, 16 that does. The result does not depend on it.
 *   HCLIB_HIP_SRAD_DAG     per iteration one reduce task R(it) (one wave, the
 *       sums in the reference's order; its promise's datum is q0sqr) and one
 *       task T(it, b) per block, which awaits R(it) and T(it - 1, b') for b and
 *       its eight in-grid neighbours (hclib_amd/csrc/hx_srad_plan.h has why this
 *       orders the overwrites of the two ping-pong grids). R(it + 1) awaits only
 *       the blocks of the region of interest.
 *   HCLIB_HIP_SRAD_PHASES  the same two bodies as one reduce kernel and one
 *       sweep kernel per iteration, stream-ordered: the form with joins, for
 *       comparison.
 * result: tasks, puts, releases from the DAG launch (phases: tasks = the
 * reduce waves and sweep workgroups run, no puts); awaits, iterations and
 * bytes_moved are the plan's; block and form as run; kernel_ms.
 * EINVAL, before the device is touched: a NULL image, a side that is not a
 * positive multiple of 16 (the reference's own check), a block outside
 * {16, 32, 64} or one that does not divide both sides, a region of interest
 * that is empty or out of range, niter < 0, an unknown form, niter (nb + 1) >=
 * 2^26 tasks or 2^32 awaits.
 * hclib_hip_srad_bounds: host only, with the same checks, exact: out[0] tasks,
 * [1] awaits, [2] the block as resolved, [3] the longest waiter list of a
 * promise, [4] the bytes of device memory, [5] bytes_moved.
 * hclib_hip_srad_image: host only: the reference's input, random_matrix
 * (srand(7), rand() / (float)RAND_MAX) followed by expf, for any rows, cols >=
 * 1. It changes the process's rand() state, as the reference does, and its
 * last bit is this host's libm's. */
typedef struct {
    uint64_t tasks, puts, releases;            /* from the DAG launch */
    uint64_t awaits, iterations, bytes_moved;  /* the plan's */
    int block, form;                           /* as run */
    double kernel_ms;                          /* device events around the launch (phases: around all iterations) */
} hclib_hip_srad_result_t;
#define HCLIB_HIP_SRAD_DAG 0
#define HCLIB_HIP_SRAD_PHASES 1
int hclib_hip_srad(const float *j0, int rows, int cols, int r1, int r2, int c1, int c2, float lambda, int niter,
                   int block, int form /* 0 dag, 1 phases */, float *j /* rows * cols */,
                   float *q0sqr /* niter, may be NULL */, hclib_hip_srad_result_t *result);
int hclib_hip_srad_image(int rows, int cols, float *j0);
int hclib_hip_srad_bounds(int rows, int cols, int r1, int r2, int c1, int c2, int niter, int block, uint64_t out[6]);

#ifdef __cplusplus
}
#endif
#endif /* HCLIB_HIP_H_ */

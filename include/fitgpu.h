/* fitgpu.h — C-ABI of the MI355X batched job→node placement engine (libfitgpu.so).
 *
 * This is the cgo seam of the new pkg/fitgpu.  The reference has no fit loop
 * of its own (capacity is summed in pkg/slurm-virtual-kubelet/node.go:169-199 and the fit runs in
 * the external kube-scheduler), so the placement entry points replace *that decision*; the
 * ingest / demand / capacity entry points replace the Go functions cited on each declaration.
 * The slurm-agent gRPC API (pkg/workload/workload.proto:23-62) and the virtual-kubelet provider
 * interface (pkg/slurm-virtual-kubelet/provider.go:26) are unchanged; INTEGRATION.md shows the
 * cgo binding and the call sites.
 *
 * Conventions
 *   - Plain pointers and sizes only.  The caller owns every buffer; the library copies inputs in
 *     during the call and never retains a caller pointer (cgo rule).
 *   - Return 0 on success, a negative FIT_E_* code on failure; fit_strerror() gives the text and
 *     fit_last_error() the detail of the last failure on the calling thread.  No C++ exception
 *     crosses the ABI.  There is no CPU fallback: without a usable gfx950 device fit_create fails.
 *   - A fit_ctx must not be used by two threads at once; several contexts may coexist.
 *   - Units: cpus, MiB, GPUs (gres/gpu count), minutes.  INT32_MAX avail = none.
 */
#ifndef FITGPU_H
#define FITGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define FITGPU_ABI_VERSION 8

/* ---- error codes ---------------------------------------------------------------------- */
#define FIT_OK 0
#define FIT_E_INVAL (-1)       /* invalid argument or input value                          */
#define FIT_E_HIP (-2)         /* HIP runtime error                                        */
#define FIT_E_RCCL (-3)        /* RCCL (collective) error                                  */
#define FIT_E_OOM (-4)         /* device or host allocation failed                         */
#define FIT_E_NODEV (-5)       /* no usable gfx950 device                                  */
#define FIT_E_STATE (-6)       /* call out of order (e.g. fit_place before fit_load_nodes) */
#define FIT_E_PARSE (-7)       /* malformed text (ingest helpers)                          */
#define FIT_E_UNLIMITED (-8)   /* ParseDuration: ErrDurationIsUnlimited                    */

/* ---- placement result codes (out_node entries) ------------------------------------------ */
#define FIT_UNPLACED (-1)  /* no node (or not enough distinct nodes) fits at this point     */
#define FIT_REJECTED (-2)  /* violates the partition's MaxTime/MaxCPUsPerNode/MaxMemPerNode  */

#define FIT_MAX_PARTITIONS 32
#define FIT_MAX_K 8         /* nodes per job (--nodes) supported by fit_place              */
#define FIT_MAX_NODES (1 << 29) /* node rows per fit_load_nodes (commit keys tag pos << 3)  */

typedef struct fit_ctx fit_ctx;

/* Optional host-side exchange used instead of RCCL (world > 1): tests run several ranks on one
 * GPU with it, a caller may route the exchange through its own transport.  In-place on host
 * memory; return 0 on success.  ops: */
#define FIT_XCHG_ALLGATHER_U64 1  /* buf holds world*count u64, this rank's block at rank*count */
#define FIT_XCHG_MIN_U64 2        /* elementwise min over ranks, count u64                    */
#define FIT_XCHG_MAX_I32 3        /* elementwise max over ranks, count int32                  */
#define FIT_XCHG_MIN_I32 4        /* elementwise min over ranks, count int32                  */
typedef int (*fit_exchange_fn)(void* user, int op, void* buf, int64_t count);

typedef struct {
    int32_t device;       /* HIP device ordinal; -1 = current device                        */
    int32_t rank;         /* this process' rank in a node-sharded group (0 if world == 1)  */
    int32_t world;        /* number of GPUs sharing one placement (1 = single GPU)         */
    const void* nccl_id;  /* 128-byte ncclUniqueId from fit_nccl_unique_id() when world>1 */
    int32_t shard_mode;   /* FIT_SHARD_*: how world > 1 ranks split one placement           */
    int32_t window_min;   /* jobs per component per round, lower bound (0 = default 256)   */
    int32_t window_max;   /* upper bound (0 = default 8192)                                 */
    int32_t flags;        /* FIT_FLAG_* bits, 0 = none                                      */
    fit_exchange_fn exchange;  /* NULL = RCCL over xGMI (nccl_id required)                  */
    void* exchange_user;
} fit_opts;

/* fit_opts.flags: run the multi-rank code path (shard split, per-round exchange, merge) even at
 * world == 1, over a one-rank RCCL communicator (or the host exchange): exercises the collective
 * calls on a single GPU.  Placements are identical to the default path. */
#define FIT_FLAG_COLLECTIVES 1

#define FIT_SHARD_AUTO 0       /* components if there are at least `world` of them, else nodes */
#define FIT_SHARD_NODES 1      /* every rank scans 1/world of every component's nodes; per     */
                               /* round: allgather candidates + 64-bit min-allreduce of bounds */
#define FIT_SHARD_COMPONENTS 2 /* ranks own whole partition components; one merge at the end   */

typedef struct {
    int64_t jobs;          /* jobs in the call                                              */
    int64_t placed;        /* jobs placed                                                    */
    int64_t unplaced;      /* FIT_UNPLACED                                                   */
    int64_t rejected;      /* FIT_REJECTED                                                   */
    int64_t rounds;        /* speculative rounds executed                                    */
    int64_t evals;         /* (job, node) fit evaluations performed by this rank's scans     */
    int64_t useful_evals;  /* J_active × N: the single-pass work of the naive scalar path    */
    int64_t stops_rescan;  /* round cut because a job's candidate list ran out               */
    int64_t stops_dirty;   /* round cut because the dirty-node set was full                  */
    double ms_total;       /* wall time of the call on the host clock                        */
    double ms_scan;        /* scan time: k_scan launches (host loop) or the average scan-   */
                           /* worker busy time inside the persistent engine                 */
    double ms_commit;      /* commit time: k_commit launches, or the slowest component's     */
                           /* committer inside the persistent engine                        */
    double ms_exchange;    /* device time in the RCCL exchange (world > 1)                   */
    double ms_device;      /* device time of the placement launches (HIP events)             */
    int32_t shard_mode;    /* mode used (FIT_SHARD_NODES / FIT_SHARD_COMPONENTS; 0 if world 1) */
    int32_t components;    /* independent partition components                               */
    int32_t engine;        /* 1: persistent single-launch engine (k_engine); 0: host-driven rounds; */
                           /* 2: direct small placement (k_small, <= FIT_SMALL_DIRECT jobs);         */
                           /* 3: demand-class engine (k_class: by default when the live jobs are at  */
                           /*    least half multi-node; FIT_CLASS=1 / 0 forces it on / off)          */
                           /* 4: multi-node backfill (fit_place_tl_k: one workgroup per component)   */
    int32_t reserved;
    double ms_arb_wait;    /* host time waiting for the device's persistent-launch lock: one   */
                           /* persistent launch per GPU at a time, across contexts and processes */
} fit_stats;

/* ---- engine -------------------------------------------------------------------------- */
int fit_create(const fit_opts* opts, fit_ctx** out_ctx);
void fit_destroy(fit_ctx* ctx);
int fit_abi_version(void);
const char* fit_strerror(int code);
const char* fit_last_error(void);
/* 128-byte RCCL unique id for a node-sharded group (rank 0 creates, everyone passes it). */
int fit_nccl_unique_id(void* out128);
/* Watchdog of the persistent engines: every device-side wait gives up after `us` microseconds
 * (default 10 s, or FIT_WATCHDOG_MS); us <= 0 restores the default.  A trip fails the call with
 * FIT_E_HIP, fit_last_error() names the wait (site, component, round, tile, ring indices, how long
 * it waited), and the context stays usable: fit_place restores the node table it started from;
 * fit_place_tl drops the timeline (FIT_E_STATE until fit_load_timeline).  Persistent launches of
 * all contexts on one GPU — in every process — run one at a time (a per-device lock file in
 * fit_lock_dir(); fit_stats.ms_arb_wait). */
int fit_set_watchdog_us(fit_ctx* ctx, int64_t us);
/* The directory of the per-GPU lock file that serialises persistent launches across processes:
 * FIT_LOCK_DIR if set; else /var/run/fitgpu when it is a directory (the hostPath volume every
 * virtual-kubelet pod of a host mounts: INTEGRATION.md item 6); else /tmp.  Writes it (NUL-
 * terminated) into buf and returns 0 when the directory is the configured or default shared one,
 * 1 when it fell back to /tmp — private to one pod in the reference's deployment (one VK pod per
 * partition, pkg/configurator/configurator.go:188-293), so VKs in other pods on the same GPU are
 * NOT arbitrated: the caller should warn.  FIT_E_INVAL: buf too small.  No device needed. */
int fit_lock_dir(char* buf, int32_t buflen);

/* Node table: one row per Slurm node, in Client.Nodes output order (pkg/slurm-agent/slurm.go:
 * 343-364); the row index is the node id placements refer to.  free = total - alloc (the
 * Node{Cpus,AlloCpus,Memory,AlloMemory,Gpus,AlloGpus} of workload.proto:165-174).  part_mask bit
 * p = member of partition p.  Host pointers. */
int fit_load_nodes(fit_ctx* ctx, int32_t n, const int32_t* cpu_free, const int32_t* mem_free,
                   const int32_t* gpu_free, const int32_t* avail_min, const uint32_t* part_mask);
/* Same, but the columns are device pointers (already resident in HBM on this context's GPU). */
int fit_load_nodes_device(fit_ctx* ctx, int32_t n, const int32_t* cpu_free,
                          const int32_t* mem_free, const int32_t* gpu_free,
                          const int32_t* avail_min, const uint32_t* part_mask);

/* Partition limits from parseResources (pkg/slurm-agent/parse.go:111-190) after the agent's
 * override merge (pkg/slurm-agent/api/slurm.go:297-341): -1 = UNLIMITED.  Minutes / CPUs / MiB. */
int fit_load_partitions(fit_ctx* ctx, int32_t p, const int32_t* max_time_min,
                        const int32_t* max_cpus_per_node, const int32_t* max_mem_per_node);

/* Place J jobs in priority order (index order) with sequential best-fit semantics.
 * Demands are per node; nodes_k (may be NULL = all 1) is the --nodes count, 0 treated as 1.
 * out_node[j*kmax + i], i < nodes_k[j]: node id, FIT_UNPLACED or FIT_REJECTED; other entries -1.
 * The context's node table is updated (jobs consume resources).  Host pointers. */
int fit_place(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
              const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, int32_t kmax,
              int32_t* out_node, fit_stats* stats);
/* Same with device pointers (inputs resident in HBM, output written in HBM). */
int fit_place_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem,
                     const int32_t* gpu, const int32_t* wall, const uint16_t* part,
                     const uint16_t* nodes_k, int32_t kmax, int32_t* out_node, fit_stats* stats);

/* Current (post-placement) free columns, in node-id order.  Host pointers, n entries each.
 * A column value that was loaded negative (the engine's own row holds max(value, -1): no job fits
 * either, so such a node never receives one) reads back exactly as it was loaded. */
int fit_read_nodes(fit_ctx* ctx, int32_t* cpu_free, int32_t* mem_free, int32_t* gpu_free);
/* Free capacity per partition (Σ over member nodes of the current free columns): the engine's
 * replacement for the allocation-blind sum of GetPartitionCapacity (node.go:183-190). */
int fit_partition_free(fit_ctx* ctx, int32_t p, int64_t* cpu, int64_t* mem_mib, int64_t* gpu);

/* ---- why a job does not fit ----------------------------------------------
 * The half of kube-scheduler's answer that fit_place does not give: its FailedScheduling event
 * ("0/5 nodes are available: 3 Insufficient cpu, 2 Insufficient memory").  fit_explain judges each
 * of J jobs ALONE against the context's current node table — the rows fit_read_nodes returns, with
 * the loaded avail_min / part_mask — and changes nothing: no job consumes anything, the order of
 * the jobs does not matter.  One 32-byte row per job. */
#define FIT_WHY_FITS 0        /* fit >= need: a fit_place of this job alone would place it now  */
#define FIT_WHY_PARTITION 1   /* part >= P (the partitions of fit_load_partitions)              */
#define FIT_WHY_LIMIT_TIME 2  /* wall > the partition's MaxTime                                  */
#define FIT_WHY_LIMIT_CPUS 3  /* cpu  > the partition's MaxCPUsPerNode                           */
#define FIT_WHY_LIMIT_MEM 4   /* mem  > the partition's MaxMemPerNode                            */
#define FIT_WHY_NO_NODES 5    /* members == 0                                                    */
#define FIT_WHY_RESOURCES 6   /* fit < need                                                      */
/* Precedence: the order above from FIT_WHY_PARTITION on (first match wins; the limits in
 * fit_place's order: time, cpus, mem), FIT_WHY_FITS last.  Codes 1-4 are exactly the jobs fit_place
 * marks FIT_REJECTED; their counters are all 0 (need is still set). */
typedef struct {
    int32_t code;        /* FIT_WHY_*                                                        */
    int32_t need;        /* nodes_k, 0 treated as 1                                          */
    int32_t members;     /* nodes with the job's partition bit set (a node whose State took  */
                         /* it out of every partition is in none)                            */
    int32_t fit;         /* members that pass all four feasibility terms now                 */
    int32_t short_cpu;   /* members with cpu_free  < cpu   — counts overlap, as kube-        */
    int32_t short_mem;   /* members with mem_free  < mem     scheduler's do: a node short of */
    int32_t short_gpu;   /* members with gpu_free  < gpu     two things is counted twice     */
    int32_t short_time;  /* members with avail_min < wall                                    */
} fit_why;
/* Host pointers; nodes_k may be NULL (= all 1).  j == 0 returns 0 whatever the pointers are.
 * FIT_E_INVAL: NULL ctx / arrays, a negative demand or nodes_k > FIT_MAX_K (the whole call fails,
 * as fit_place's does).  FIT_E_STATE: before fit_load_nodes; while a timeline is loaded (the
 * backfill view is fit_when's, or fit_place_tl's start slot); on a context created with world > 1 or
 * FIT_FLAG_COLLECTIVES (a rank holds no whole answer).  Three bounded launches, no persistent
 * grid: the call neither takes the per-GPU persistent-launch lock nor needs the watchdog. */
int fit_explain(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, fit_why* out);
/* Same with device pointers (inputs resident in HBM, the rows written in HBM). */
int fit_explain_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem,
                       const int32_t* gpu, const int32_t* wall, const uint16_t* part,
                       const uint16_t* nodes_k, fit_why* out);
/* Diagnostic, for measurement only (tools/explain_bench.py): device time of the last successful
 * fit_explain_device on this context, in milliseconds — HIP events on the context's own stream
 * around its launches, which a caller cannot record from outside.  FIT_E_STATE when there has
 * been none. */
int fit_explain_ms(fit_ctx* ctx, double* ms);
/* The row as one line of text in kube-scheduler's shape, NUL-terminated into buf.  Host only: no
 * device, no context.  Returns the length written (without the NUL), or FIT_E_INVAL: NULL
 * arguments, an unknown code, or a buffer too small for the text and its NUL (256 bytes always
 * suffice).  The exact texts, <x> a decimal field of the row:
 *   FIT_WHY_FITS        "<fit>/<members> nodes fit now"
 *   FIT_WHY_RESOURCES   "<fit>/<members> nodes fit now: <short_cpu> insufficient cpu,
 *                        <short_mem> insufficient memory, <short_gpu> insufficient gpu,
 *                        <short_time> not available for the walltime"
 *                       — on one line, terms joined by ", "; a term whose count is 0 is left out,
 *                       and with no term left the ": " goes too
 *     both with " (need <need>)" after "now" when need > 1, e.g.
 *     "0/6273 nodes fit now (need 2): 5120 insufficient cpu, 73 insufficient memory"
 *   FIT_WHY_NO_NODES    "no schedulable node in the partition"
 *   FIT_WHY_LIMIT_TIME  "walltime exceeds the partition's MaxTime"
 *   FIT_WHY_LIMIT_CPUS  "cpus per node exceed the partition's MaxCPUsPerNode"
 *   FIT_WHY_LIMIT_MEM   "memory per node exceeds the partition's MaxMemPerNode"
 *   FIT_WHY_PARTITION   "unknown partition" */
int fit_why_message(const fit_why* w, char* buf, int32_t buflen);

/* ---- time-windowed backfill (BASELINE config C5) -------------------------
 * Each node's free resources over a horizon of `slots` slots of `slot_min` minutes (slots <=
 * 1024): the node table of the last fit_load_nodes is the state at slot 0, and the jobs already
 * running hand resources back at their end — release events, CSR by node id: node x's events are
 * [rel_off[x], rel_off[x+1]) with non-decreasing rel_slot (slot <= 0 = already free) and amounts
 * >= 0.  A node is usable for slots t < avail_min / slot_min.  Call after fit_load_nodes (which
 * drops the timeline); rel_off NULL = no releases.  Host pointers; rel_off has n+1 entries.
 * At most 2^22 - 1 nodes with a partition bit (the backfill key's position field): FIT_E_INVAL.
 * The walltime source is the job's --time (pkg/slurm-bridge-operator/parse.go:84-91) and the
 * squeue EndTime of running jobs; the partition MaxTime check is parseResources' (parse.go:128-138). */
int fit_load_timeline(fit_ctx* ctx, int32_t slots, int32_t slot_min, const int32_t* rel_off,
                      const int32_t* rel_slot, const int32_t* rel_cpu, const int32_t* rel_mem,
                      const int32_t* rel_gpu);
/* Same with device pointers; n_rel = rel_off[n] (the caller knows it; not read back). */
int fit_load_timeline_device(fit_ctx* ctx, int32_t slots, int32_t slot_min,
                             const int32_t* rel_off, int64_t n_rel, const int32_t* rel_slot,
                             const int32_t* rel_cpu, const int32_t* rel_mem,
                             const int32_t* rel_gpu);
/* Sequential priority-order backfill: each job (one node, nodes_k = 1) gets the node and the
 * earliest start slot at which its demand fits for ceil(wall / slot_min) consecutive slots, best
 * fit among the nodes with that start; the reservation is committed and later
 * jobs see it.  out_node[j]: node id, FIT_UNPLACED (no start inside the horizon) or FIT_REJECTED;
 * out_start[j]: start slot, -1 when not placed.  Host pointers.  Jobs of several nodes on the
 * timeline: fit_place_tl_k below. */
int fit_place_tl(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem,
                 const int32_t* gpu, const int32_t* wall, const uint16_t* part, int32_t* out_node,
                 int32_t* out_start, fit_stats* stats);
/* Same with device pointers (inputs resident in HBM, outputs written in HBM). */
int fit_place_tl_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem,
                        const int32_t* gpu, const int32_t* wall, const uint16_t* part,
                        int32_t* out_node, int32_t* out_start, fit_stats* stats);
/* Release events for fit_load_timeline from the running jobs a caller knows — the virtual
 * kubelet's own pods: JobInfo.end_time and JobInfo.node_list (workload.proto:252-292; the
 * node_list expanded with fit_expand_hostlist and mapped to engine rows through the
 * fit_node_names table) and each pod's per-node demand (fit_pod_demand).  Job i holds (cpu[i],
 * mem[i], gpu[i]) on every node job_nodes[job_off[i] .. job_off[i+1]) for rem_min[i] more minutes
 * (end_time − now) and hands it back at slot max(1, ceil(rem_min / slot_min)), capped at `slots`
 * (a job past its end time holds its nodes until Slurm ends it; a release at the horizon changes
 * nothing).  Output: the CSR by node fit_load_timeline reads (rel_off[n + 1]; rel_slot / rel_cpu /
 * rel_mem / rel_gpu, slots non-decreasing per node, jobs in order within a slot), at most cap
 * events.  Returns the event count or FIT_E_INVAL (node id out of range, negative demand,
 * job_off not starting at 0 or decreasing, slots / slot_min < 1, cap too small). */
int fit_release_events(int32_t n, int32_t m, const int32_t* job_off, const int32_t* job_nodes,
                       const int64_t* rem_min, const int32_t* cpu, const int32_t* mem,
                       const int32_t* gpu, int32_t slots, int32_t slot_min, int32_t* rel_off,
                       int32_t* rel_slot, int32_t* rel_cpu, int32_t* rel_mem, int32_t* rel_gpu,
                       int32_t cap);
/* Current timelines, dense [n][slots] per column, host pointers (n * slots entries each).  Slots
 * where a node is unusable, and nodes outside every partition, read -1. */
int fit_read_timeline(fit_ctx* ctx, int32_t* cpu, int32_t* mem, int32_t* gpu);

/* ---- when a pending job can start -----------------------------------------
 * The backfill half of fit_explain's answer — `squeue --start`, `sbatch --test-only`: fit_when
 * judges each of J jobs ALONE against the context's current timeline — the one fit_load_timeline
 * built, minus every reservation fit_place_tl has committed since: what fit_read_timeline returns —
 * and changes nothing: nothing is reserved, the order of the jobs does not matter.  A job takes one
 * node (§2b).  One 32-byte row per job. */
#define FIT_ETA_NOW 0         /* start == 0: a fit_place_tl of this job alone would start it now  */
#define FIT_ETA_PARTITION 1   /* = FIT_WHY_PARTITION    these four: FIT_WHY_*'s numbers, rule and */
#define FIT_ETA_LIMIT_TIME 2  /* = FIT_WHY_LIMIT_TIME   order — exactly the jobs fit_place_tl     */
#define FIT_ETA_LIMIT_CPUS 3  /* = FIT_WHY_LIMIT_CPUS   marks FIT_REJECTED                        */
#define FIT_ETA_LIMIT_MEM 4   /* = FIT_WHY_LIMIT_MEM                                              */
#define FIT_ETA_NO_NODES 5    /* members == 0 (= FIT_WHY_NO_NODES)                                */
#define FIT_ETA_LATER 6       /* start > 0                                                        */
#define FIT_ETA_HORIZON 7     /* hosts == 0: no node has a start inside the horizon (dur > slots  */
                              /* is one way to get here)                                          */
/* Precedence: 1, 2, 3, 4, 5, 7, 6, 0 (first match wins).  For codes 1-4 every field but code and
 * dur is 0, with start = node = wait_min = -1. */
typedef struct {
    int32_t code;      /* FIT_ETA_*                                                            */
    int32_t dur;       /* max(1, ceil(wall / slot_min)) slots; set for every code             */
    int32_t start;     /* the smallest earliest start slot over the members, -1 if none       */
    int32_t node;      /* the node of the smallest §2b key (earliest start, then best fit,    */
                       /* then node id), -1 if none: what fit_place_tl of this job alone      */
                       /* would return                                                        */
    int32_t wait_min;  /* start * slot_min, saturated at INT32_MAX; -1 if none                */
    int32_t members;   /* nodes with the job's partition bit set                              */
    int32_t hosts;     /* members that have any start inside the horizon                      */
    int32_t now;       /* members whose earliest start is slot 0                              */
} fit_eta;
/* Host pointers.  j == 0 returns 0 whatever the pointers are.  FIT_E_INVAL: NULL ctx / arrays,
 * j < 0, a negative demand (the whole call fails, as fit_place_tl's does).  FIT_E_STATE: before
 * fit_load_nodes; without a timeline loaded; on a context created with world > 1 or
 * FIT_FLAG_COLLECTIVES (a rank holds no whole answer).  Three bounded launches, no persistent grid:
 * the call neither takes the per-GPU persistent-launch lock nor needs the watchdog. */
int fit_when(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
             const int32_t* wall, const uint16_t* part, fit_eta* out);
/* Same with device pointers (inputs resident in HBM, the rows written in HBM). */
int fit_when_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                    const int32_t* wall, const uint16_t* part, fit_eta* out);
/* Diagnostic, for measurement only (tools/when_bench.py): device time of the last successful
 * fit_when_device on this context, in milliseconds (HIP events on the context's own stream around
 * its launches).  FIT_E_STATE when there has been none. */
int fit_when_ms(fit_ctx* ctx, double* ms);
/* The row as one line of text, NUL-terminated into buf.  Host only: no device, no context.
 * Returns the length written (without the NUL), or FIT_E_INVAL: NULL arguments, an unknown code,
 * or a buffer too small for the text and its NUL (256 bytes always suffice).  The exact texts,
 * <x> a decimal field of the row:
 *   FIT_ETA_NOW         "can start now on <now>/<members> nodes"
 *   FIT_ETA_LATER       "earliest start in <wait_min> min (slot <start>): <hosts>/<members> nodes
 *                        can run it inside the horizon, none now"   — on one line
 *   FIT_ETA_HORIZON     "no start inside the horizon on any of <members> nodes"
 *   FIT_ETA_NO_NODES / LIMIT_TIME / LIMIT_CPUS / LIMIT_MEM / PARTITION: fit_why_message's texts of
 *                       the codes with the same numbers, verbatim */
int fit_when_message(const fit_eta* e, char* buf, int32_t buflen);

/* ---- when a multi-node job can start ---------------------------------------
 * fit_when for jobs of nodes_k nodes: the earliest slot at which need = max(nodes_k, 1) DISTINCT
 * member nodes all hold the demand over the same d slots, and the need best-fitting of the nodes
 * free there.  Judged alone against the current timeline, read-only, as fit_when.  With S_n the set
 * of slots s (s + d <= slots) from which node n holds (cpu, mem, gpu) on every slot of [s, s + d),
 * cnt(s) is the number of members with s in S_n.  The common start can be later than every node's
 * own earliest start: the k-th smallest of fit_when's per-node starts is not the answer.  For
 * need == 1 start, the node and the counters are fit_when's.  The codes are FIT_ETA_*, numbers and
 * precedence unchanged; FIT_ETA_HORIZON here means no s has cnt(s) >= need (hosts < need and
 * dur > slots are two ways to get there).  For codes 1-4 every field but code, dur and need is 0,
 * with start = wait_min = -1.  One 40-byte row per job. */
typedef struct {
    int32_t code;      /* FIT_ETA_*                                                            */
    int32_t dur;       /* max(1, ceil(wall / slot_min)) slots; set for every code             */
    int32_t need;      /* nodes_k, 0 treated as 1; set for every code                         */
    int32_t start;     /* the smallest s with cnt(s) >= need, -1 if none                      */
    int32_t wait_min;  /* start * slot_min, saturated at INT32_MAX; -1 if none                */
    int32_t members;   /* nodes with the job's partition bit set                              */
    int32_t hosts;     /* members that have any start inside the horizon                      */
    int32_t now;       /* cnt(0): members that hold the demand from slot 0                    */
    int32_t ready;     /* cnt(start): members that hold it from `start`; 0 if none            */
    int32_t reserved;  /* 0                                                                   */
} fit_eta_k;
/* Host pointers; nodes_k may be NULL (= all 1).  out_node has j * kmax entries: when the code is
 * FIT_ETA_NOW or FIT_ETA_LATER, out_node[j * kmax + i], i < need, are the need smallest (score,
 * node id) among the members that hold the demand from `start`, in that order — the score is
 * fit_place's packing of the window minima minus the demand; every other entry is -1.  j == 0
 * returns 0 whatever the pointers are.  FIT_E_INVAL: NULL ctx / arrays, j < 0, kmax < 1 or kmax >
 * FIT_MAX_K, any max(nodes_k, 1) > kmax, any negative demand (the whole call fails).  FIT_E_STATE:
 * before fit_load_nodes; without a timeline loaded; on a context created with world > 1 or
 * FIT_FLAG_COLLECTIVES.  Bounded launches per chunk of 16,384 jobs, no persistent grid: the call
 * neither takes the per-GPU persistent-launch lock nor needs the watchdog. */
int fit_when_k(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
               const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, int32_t kmax,
               fit_eta_k* out, int32_t* out_node);
/* Same with device pointers (inputs resident in HBM, rows and nodes written in HBM). */
int fit_when_k_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                      const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, int32_t kmax,
                      fit_eta_k* out, int32_t* out_node);
/* Diagnostic, for measurement only (tools/when_k_bench.py): device time of the last successful
 * fit_when_k_device on this context, in milliseconds (HIP events on the context's own stream around
 * its launches).  FIT_E_STATE when there has been none. */
int fit_when_k_ms(fit_ctx* ctx, double* ms);
/* The row as one line of text, NUL-terminated into buf.  Host only: no device, no context.
 * Returns the length written (without the NUL), or FIT_E_INVAL: NULL arguments, an unknown code,
 * or a buffer too small for the text and its NUL (256 bytes always suffice).  The exact texts,
 * <x> a decimal field of the row:
 *   FIT_ETA_NOW         "can start now on <need> of <ready>/<members> nodes"
 *   FIT_ETA_LATER       "earliest start in <wait_min> min (slot <start>) on <need> of
 *                        <ready>/<members> nodes, <now> free now"   — on one line
 *   FIT_ETA_HORIZON     "no start inside the horizon for <need> nodes at once: <hosts>/<members>
 *                        nodes can run it"   — on one line
 *   FIT_ETA_NO_NODES / LIMIT_TIME / LIMIT_CPUS / LIMIT_MEM / PARTITION: fit_why_message's texts of
 *                       the codes with the same numbers, verbatim */
int fit_when_k_message(const fit_eta_k* e, char* buf, int32_t buflen);

/* ---- begin and deadline per job: the multi-node pair with a window ------------
 * fit_when_k and fit_place_tl_k search the whole horizon from slot 0.  The two calls below take two
 * more optional job columns — `sbatch --begin` / `--deadline`, the planned end of a dependency's
 * parent, the recorded start of a row fit_hold_tl refused — and are otherwise §2f / §2g word for
 * word.  Per job, with H the timeline's slots and d = max(1, ceil(wall / slot_min)):
 *   from  = clamp(not_before, 0, H)       until = clamp(deadline, 0, H)
 *   A     = { s : from <= s and s + d <= until }       the allowed starts
 * No value of either column is an error: a negative not_before is 0 (what is left of a begin time
 * after subtracting fit_advance_tl's `a`), a deadline <= 0 has passed, a deadline >= H (INT32_MAX)
 * is none.  S_n, cnt(s), the score, the node order and the partition rejections are fit_when_k's;
 * `start` is the smallest s in A with cnt(s) >= need, the nodes are the need smallest (score, node
 * id) among the members with start in S_n, the score from the minima over [start, start + d) only.
 * The row is a fit_eta_k:
 *   hosts   members with S_n ∩ A not empty
 *   now     cnt(from) if from is in A, else 0: the nodes free at the job's earliest allowed start
 *   ready   cnt(start); members, dur, need, wait_min as fit_when_k's
 * Codes 1-5 as fit_when_k, same precedence; with a start FIT_ETA_NOW when start == 0, else
 * FIT_ETA_LATER; without one FIT_ETA_HORIZON when A is the whole range (from == 0 and until == H),
 * else FIT_ETA_WINDOW.  Code 8 comes from fit_when_k_win alone; fit_when_message and
 * fit_when_k_message refuse it.  With both columns NULL, or any columns that clamp to (0, H), rows
 * and nodes equal fit_when_k's field for field.  If fit_when_k's start lies in A, start and nodes
 * are fit_when_k's.  Not here: dependencies INSIDE one call (a parent may sit in another partition
 * component, whose jobs are placed concurrently: chain two calls, not_before = out_start + dur of
 * the parent), and windows for fit_when / fit_place_tl (nodes_k <= 1 here gives their answers). */
#define FIT_ETA_WINDOW 8 /* no s in A has cnt(s) >= need, and A is not the whole range */
/* Host pointers; nodes_k, not_before and deadline may each be NULL (all 1 / all 0 / none).  out,
 * out_node, j == 0, FIT_E_INVAL, FIT_E_STATE and the launches are fit_when_k's: read-only, bounded
 * launches per chunk of 16,384 jobs, no lock, no watchdog.  A job whose A is empty walks nothing. */
int fit_when_k_win(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                   const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, int32_t kmax,
                   const int32_t* not_before /* j; NULL = all 0 */, const int32_t* deadline /* j; NULL = none */,
                   fit_eta_k* out, int32_t* out_node);
/* Same with device pointers (inputs resident in HBM, rows and nodes written in HBM). */
int fit_when_k_win_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                          const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, int32_t kmax,
                          const int32_t* not_before, const int32_t* deadline, fit_eta_k* out,
                          int32_t* out_node);
/* Diagnostic, for measurement only (tools/win_tl_bench.py): device time of the last successful
 * fit_when_k_win_device on this context, in milliseconds.  FIT_E_STATE when there has been none. */
int fit_when_k_win_ms(fit_ctx* ctx, double* ms);
/* The row as one line of text, as fit_when_k_message (same returns, 256 bytes always suffice):
 *   FIT_ETA_WINDOW      "no start inside its window for <need> nodes at once: <hosts>/<members>
 *                        nodes can run it there"   — on one line
 *   every other code    fit_when_k_message's text, verbatim */
int fit_when_k_win_message(const fit_eta_k* e, char* buf, int32_t buflen);

/* ---- priority-order backfill of multi-node jobs -----------------------------
 * fit_place_tl for jobs of nodes_k nodes, the committing half of fit_when_k: jobs 0 .. j-1 in
 * index order, each judged against the timeline AS THE JOBS BEFORE IT LEFT IT.  Partition
 * rejection is fit_place_tl's (FIT_REJECTED, nothing consumed).  Otherwise, with need =
 * max(nodes_k, 1) and d = max(1, ceil(wall / slot_min)): the start is the smallest s with cnt(s) >=
 * need, the nodes are the need smallest (score, node id) among the members free from it —
 * fit_when_k's row and node list, field for field — and (cpu, mem, gpu) is subtracted on slots
 * [start, start + d) of EACH of them: a gang reserves on need nodes or on none.  Without a start the
 * job is FIT_UNPLACED and consumes nothing.  A queue with every nodes_k <= 1 gives fit_place_tl's
 * nodes, starts and timeline; job 0's result is fit_when_k's answer on the timeline as loaded; the
 * node table (fit_read_nodes) is untouched.
 * Host pointers; nodes_k may be NULL (= all 1); stats may be NULL.  out_node has j * kmax entries:
 * out_node[q * kmax + i], i < need, are a placed job's nodes in key order and every other entry is
 * -1; a rejected job has out_node[q * kmax] = FIT_REJECTED and the rest -1; an unplaced job has all
 * entries -1 (FIT_UNPLACED).  out_start[q]: the start slot, -1 when the job is not placed.  j == 0
 * returns 0 whatever the pointers are and zeroes stats.
 * FIT_E_INVAL: NULL ctx / arrays, j < 0, kmax < 1 or kmax > FIT_MAX_K, any max(nodes_k, 1) > kmax,
 * any negative demand — the whole call fails and the timeline is unchanged (the batch is validated
 * before the first reservation).  FIT_E_STATE: before fit_load_nodes; without a timeline loaded; on a
 * context created with world > 1 or FIT_FLAG_COLLECTIVES.  A HIP error once reservations have begun
 * drops the timeline, as a watchdog trip of fit_place_tl does: FIT_E_STATE until fit_load_timeline.
 * stats: jobs, placed, unplaced, rejected, components, ms_total, ms_device (HIP events on the
 * context's stream) and engine = 4; every other field is 0 (ms_arb_wait too: no lock is taken).
 * Bounded launches, one workgroup per partition component, at most 16,384 jobs of a component per
 * launch; no persistent grid: the call neither takes the per-GPU persistent-launch lock nor needs
 * the watchdog.  One workgroup walks a component's nodes per job, so a table that is a single large
 * component is slow. */
int fit_place_tl_k(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                   const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, int32_t kmax,
                   int32_t* out_node /* j * kmax */, int32_t* out_start /* j */, fit_stats* stats);
/* Same with device pointers (inputs resident in HBM, outputs written in HBM). */
int fit_place_tl_k_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                          const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, int32_t kmax,
                          int32_t* out_node /* j * kmax */, int32_t* out_start /* j */, fit_stats* stats);
/* fit_place_tl_k with fit_when_k_win's start rule: the queue runs in index order,
 * each job judged against the timeline as the jobs before it left it, its start the smallest s in
 * its own A with cnt(s) >= need, the reservation all-or-nothing on [start, start + d) of each node.
 * A job without an allowed start is FIT_UNPLACED and consumes nothing, so the jobs behind it are
 * never judged against a reservation outside its window.  Every placed job has from <= start and
 * start + d <= until.  Job 0's result is fit_when_k_win's answer on the timeline as loaded; with
 * both columns NULL, or any that clamp to (0, H), nodes, starts, stats and the final timeline are
 * fit_place_tl_k's.  fit_unplace_tl of the outputs restores the timeline bit for bit, and after a
 * reload fit_hold_tl of them holds every row.  Outputs, stats (engine = 4), j == 0, errors, state
 * rules and launches are fit_place_tl_k's; a failed call leaves the timeline byte-identical.
 * Host pointers; nodes_k, not_before, deadline and stats may each be NULL. */
int fit_place_tl_k_win(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                       const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, int32_t kmax,
                       const int32_t* not_before /* j; NULL = all 0 */, const int32_t* deadline /* j; NULL = none */,
                       int32_t* out_node /* j * kmax */, int32_t* out_start /* j */, fit_stats* stats);
/* Same with device pointers (inputs resident in HBM, outputs written in HBM). */
int fit_place_tl_k_win_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                              const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, int32_t kmax,
                              const int32_t* not_before, const int32_t* deadline, int32_t* out_node /* j * kmax */,
                              int32_t* out_start /* j */, fit_stats* stats);

/* ---- hand reservations back to the timeline ---------------------------------
 * The inverse of fit_place_tl / fit_place_tl_k, for a deleted pod or a running job that ends
 * before its end_time: demand windows are ADDED to the current timeline (what fit_read_timeline
 * returns).  Row q is one job in the columns a caller gave to, and got from, fit_place_tl_k:
 * per-node demand (cpu, mem, gpu)[q], wall[q], nodes_k[q], node[q * kmax + i] and start[q]; with
 * kmax = 1 and nodes_k = NULL they are fit_place_tl's.  A row with start[q] < 0 is skipped whatever
 * else it holds, so a placement's outputs go back verbatim, unplaced and rejected rows included.
 * A live row, with need = max(nodes_k, 1) and d = max(1, ceil(wall / slot_min)), covers slots
 * [start, min(start + d, H)) of each of node[q * kmax .. + need); entries i >= need are ignored.
 * Per slot and column a value of -1 stays -1 (unusable slot, node in no partition, column loaded
 * negative: nothing was ever reserved there) and any other value v becomes min(v + demand,
 * INT32_MAX).  Both rules commute and associate: the result does not depend on the order of the
 * rows, and two calls give what one gives.  Run lists stay canonical and the node headers follow.
 * Unplacing every placed row of a placement restores the timeline it started from, bit for bit;
 * start = 0, wall = rem_min on a running job's nodes removes it from the loaded timeline (as long
 * as no value was clamped).  The node table (fit_read_nodes) is untouched.
 * Host pointers; nodes_k may be NULL (= all 1); *applied (may be NULL) is the number of (row, node)
 * windows added: the sum of need over the live rows.  j == 0 returns 0 whatever the pointers are.
 * FIT_E_INVAL: NULL ctx / arrays, j < 0, kmax < 1 or kmax > FIT_MAX_K; in a live row a negative
 * demand, need > kmax, start >= H, a node id outside [0, n) or the same node twice — the whole call
 * fails and the timeline is unchanged (the batch is validated before the first write).
 * FIT_E_STATE: before fit_load_nodes; without a timeline loaded; on a context created with world > 1
 * or FIT_FLAG_COLLECTIVES.  A HIP error once writing has begun drops the timeline, as in
 * fit_place_tl_k: FIT_E_STATE until fit_load_timeline.
 * Bounded launches, one wave per touched node, at most 16,384 rows per launch sequence; no
 * persistent grid: the call neither takes the per-GPU persistent-launch lock nor needs the
 * watchdog. */
int fit_unplace_tl(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                   const int32_t* wall, const uint16_t* nodes_k /* NULL = all 1 */, int32_t kmax,
                   const int32_t* node /* j * kmax */, const int32_t* start /* j */,
                   int64_t* applied /* may be NULL: (row, node) windows added */);
/* Same with device pointers (inputs resident in HBM); applied is a host pointer. */
int fit_unplace_tl_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                          const int32_t* wall, const uint16_t* nodes_k, int32_t kmax, const int32_t* node,
                          const int32_t* start, int64_t* applied);
/* Device time (HIP events) of the last successful fit_unplace_tl / fit_unplace_tl_device, as
 * fit_when_k_ms; FIT_E_STATE before the first. */
int fit_unplace_tl_ms(fit_ctx* ctx, double* ms);

/* ---- move the timeline forward with the clock --------------------------------
 * Slot 0 is "now" at the time of fit_load_timeline.  After a slots of slot_min minutes have passed,
 * a running job's release slot ceil(rem_min / slot_min) and every reservation lie a slots earlier:
 * the correct timeline is the old one moved left by a, plus a new slots at the far end.  With T the
 * current dense timeline (what fit_read_timeline returns), H the loaded horizon and a' = min(a, H),
 * per node n and per column:
 *   T'[n][t] = T[n][t + a']                      for t < H - a';
 *   for t >= H - a':  -1 if T[n][H - 1] == -1 in that column (a node past its avail_min, a column
 *   loaded negative and a node in no partition stay unusable whatever the tail says, so a caller may
 *   pass the same plain level for every node), otherwise tail_col[n], which must be >= -1 (-1 makes
 *   the new slots unusable in that column).
 * tail_cpu / tail_mem / tail_gpu: n entries each in the caller's node order — per node, its total
 * minus the demand of the running jobs that end beyond the new horizon.  With all three NULL every
 * column continues its slot H - 1 value; that is exact only when no reservation and no pending
 * release reaches the old horizon edge (slot H - 1 then holds the node's plain level), and it does
 * not commute with fit_unplace_tl of a window that touches slot H - 1.
 * a == 0 returns 0 and changes nothing, whatever the pointers are.  The node table (fit_read_nodes),
 * H, slot_min and the partitions are untouched.  Run lists stay canonical (the tail joins the last
 * surviving run when all three columns agree; at most H - a' + 1 runs), cnt and head[] are
 * refreshed and every header ceiling is recomputed exactly from the runs written — the only
 * operation that lowers a ceiling on a timeline that lives for days.
 * advance(a, tail) then advance(b, tail) equals advance(a + b, tail) for explicit tails; with
 * explicit tails the call commutes with fit_unplace_tl: unplacing a window [s, e), e = min(s + d, H),
 * before the advance equals unplacing [max(s - a', 0), e - a') after it, windows with e <= a' dropped
 * (start' = max(start - a, 0), wall' = (e - a - start') * slot_min).
 * FIT_E_INVAL: NULL ctx, a < 0, some but not all tail pointers NULL, a tail value < -1 — the whole
 * call fails and the timeline is unchanged (the tails are validated before the first write).
 * FIT_E_STATE: before fit_load_nodes; without a timeline loaded; on a context created with world > 1
 * or FIT_FLAG_COLLECTIVES.  A HIP error once writing has begun drops the timeline, as in
 * fit_place_tl_k: FIT_E_STATE until fit_load_timeline.
 * Every node with a run list is touched, in place, one wave per list; bounded launches, no
 * persistent grid: the call neither takes the
 * per-GPU persistent-launch lock nor needs the watchdog. */
int fit_advance_tl(fit_ctx* ctx, int32_t a, const int32_t* tail_cpu, const int32_t* tail_mem,
                   const int32_t* tail_gpu /* host pointers, n entries, caller's node order; all NULL: continue */);
/* Same with device pointers (tails resident in HBM). */
int fit_advance_tl_device(fit_ctx* ctx, int32_t a, const int32_t* tail_cpu, const int32_t* tail_mem,
                          const int32_t* tail_gpu);
/* Device time (HIP events) of the last successful fit_advance_tl / fit_advance_tl_device with a > 0,
 * as fit_unplace_tl_ms; FIT_E_STATE before the first. */
int fit_advance_tl_ms(fit_ctx* ctx, double* ms);

/* ---- re-apply recorded reservations to the timeline -------------------------
 * The committing mirror of fit_unplace_tl, for the placement records a caller kept across a
 * reload (fit_load_nodes + fit_load_timeline after a resync, a dropped timeline, a restart):
 * demand windows are SUBTRACTED from the current timeline (what fit_read_timeline returns) at their
 * RECORDED nodes and start slots — nothing is chosen again — and the caller learns which records no
 * longer fit.  The rows are fit_unplace_tl's, field for field: a row with start[q] < 0 is skipped
 * whatever else it holds and gets FIT_HOLD_SKIPPED; a live row, with need = max(nodes_k, 1) and
 * d = max(1, ceil(wall / slot_min)), covers slots [start, min(start + d, H)) of each of
 * node[q * kmax .. + need); entries i >= need are ignored.  No partition, limit or membership test
 * is made: the caller vouches for a record it got from a placement.
 * Judging is ONE pass over the timeline T as the call found it, with ALL live rows of the call
 * counted, whatever j is: S[n][t][c] is the exact sum (it does not wrap: three rows of INT32_MAX
 * compare as larger than INT32_MAX) of the demands of all live windows that cover slot t of node n
 * in column c; slot (n, t) is over iff S > T in any column, so a slot that reads -1 in any column
 * (past avail_min, a column loaded negative, a node in no partition) is over for every window that
 * covers it, a zero demand included — fit_place_tl's feasibility test, v >= demand.  A live row is
 * refused (FIT_HOLD_REFUSED) iff any slot of any of its windows is over, else held (FIT_HOLD_HELD).
 * There is no fixpoint: a row refused because of node A still counts on its node B and can make a
 * row there refused too, and all parties of a conflict are refused, not the later one.  So the
 * outcome, out_state included, does not depend on the order of the rows; the caller hands the
 * refused rows to fit_place_tl_k, which resolves them in priority order.
 * Only the held rows are applied: T' = T - S_held.  S_held <= S <= T on every slot a held window
 * covers, so nothing clamps, no value goes below 0 and no -1 slot is touched.  Run lists stay
 * canonical; cnt, head[] and the ceilings of every node a held window touches are refreshed, the
 * ceilings exactly.  The node table (fit_read_nodes) is untouched.
 * Replaying a placement's outputs verbatim on the timeline it started from gives, bit for bit, the
 * timeline it ended with, every placed row held.  fit_unplace_tl of exactly the held rows restores
 * the timeline the hold found, bit for bit.  When no row is refused, two calls give what one gives.
 * Host pointers; nodes_k may be NULL (= all 1); *applied (may be NULL) is the sum of need over the
 * held rows, *refused (may be NULL) the number of refused rows.  j == 0 returns 0 whatever the
 * pointers are.
 * FIT_E_INVAL: NULL ctx / arrays (out_state included), j < 0, kmax < 1 or kmax > FIT_MAX_K; in a
 * live row a negative demand, need > kmax, start >= H, a node id outside [0, n) or the same node
 * twice — the whole call fails, the timeline and out_state are unchanged (the batch is validated
 * before the first write).
 * FIT_E_STATE: before fit_load_nodes; without a timeline loaded; on a context created with world > 1
 * or FIT_FLAG_COLLECTIVES.  A HIP error once writing has begun drops the timeline, as in
 * fit_place_tl_k: FIT_E_STATE until fit_load_timeline.
 * Bounded launches, two passes of one wave per touched node over the windows of the whole call
 * (32 B of scratch per window); no persistent grid: the call neither takes the per-GPU
 * persistent-launch lock nor needs the watchdog. */
#define FIT_HOLD_HELD     1
#define FIT_HOLD_REFUSED  0
#define FIT_HOLD_SKIPPED (-1)
int fit_hold_tl(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                const int32_t* wall, const uint16_t* nodes_k /* NULL = all 1 */, int32_t kmax,
                const int32_t* node /* j * kmax */, const int32_t* start /* j */,
                int32_t* out_state /* j */, int64_t* applied /* may be NULL */, int64_t* refused /* may be NULL */);
/* Same with device pointers (inputs resident in HBM, out_state written in HBM); applied and refused
 * are host pointers. */
int fit_hold_tl_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                       const int32_t* wall, const uint16_t* nodes_k, int32_t kmax, const int32_t* node,
                       const int32_t* start, int32_t* out_state, int64_t* applied, int64_t* refused);
/* Device time (HIP events) of the last successful fit_hold_tl / fit_hold_tl_device, as
 * fit_unplace_tl_ms; FIT_E_STATE before the first. */
int fit_hold_tl_ms(fit_ctx* ctx, double* ms);

/* ---- how many more copies of a job fit now ---------------------------------
 * The count fit_explain does not give — "room for 12 of its 40 array tasks now", the pods a
 * partition takes of one shape, the resource that runs out first: fit_room judges each of J jobs
 * ALONE against the context's current node table, as fit_explain does, and changes nothing.  A job
 * is its per-node demand; there is no nodes_k (for a k-node job the row counts node shares: the
 * largest number of k-node jobs is not floor(copies / k), §2e).  On a feasible member node
 * (fit_explain's four terms) `per` = min over the resources r in {gpu, cpu, mem} with demand_r > 0
 * of floor(free_r / demand_r), FIT_ROOM_UNBOUNDED if all three demands are 0; on any other node
 * per = 0.  The binding resource of a feasible node is the first r in the order gpu, cpu, mem with
 * demand_r > 0 and floor(free_r / demand_r) == per.  One 40-byte row per job. */
#define FIT_ROOM_SOME 0        /* copies > 0: a fit_place of m one-node copies of this job alone   */
                               /* places min(m, copies) of them                                     */
#define FIT_ROOM_PARTITION 1   /* = FIT_WHY_PARTITION    these four: FIT_WHY_*'s numbers, rule and */
#define FIT_ROOM_LIMIT_TIME 2  /* = FIT_WHY_LIMIT_TIME   order; every other field is 0, with       */
#define FIT_ROOM_LIMIT_CPUS 3  /* = FIT_WHY_LIMIT_CPUS   best_node = -1                            */
#define FIT_ROOM_LIMIT_MEM 4   /* = FIT_WHY_LIMIT_MEM                                              */
#define FIT_ROOM_NO_NODES 5    /* members == 0 (= FIT_WHY_NO_NODES)                                */
#define FIT_ROOM_NONE 6        /* copies == 0                                                      */
#define FIT_ROOM_UNBOUNDED 2147483647 /* per of a feasible node for an all-zero demand (INT32_MAX) */
/* Precedence: 1, 2, 3, 4, 5, 6, 0 (first match wins).  The row and the call share a name, so the
 * row is a struct tag: `struct fit_room` in C and in C++. */
struct fit_room {
    int32_t code;       /* FIT_ROOM_*                                                          */
    int32_t members;    /* as fit_why.members                                                  */
    int32_t nodes;      /* feasible members; equals fit_why.fit                                */
    int32_t best;       /* max of per over the members, 0 if none                              */
    int64_t copies;     /* sum of per over the members (64 bits: cannot overflow)              */
    int32_t best_node;  /* node id of a node with per == best > 0, the lowest on a tie; -1 if  */
                        /* none                                                                */
    int32_t by_gpu;     /* feasible members whose binding resource is gpu                      */
    int32_t by_cpu;     /*   ... cpu                                                           */
    int32_t by_mem;     /*   ... memory; the three sum to nodes, or are 0 for an all-zero      */
                        /* demand                                                              */
};
/* Host pointers.  j == 0 returns 0 whatever the pointers are.  FIT_E_INVAL: NULL ctx / arrays,
 * j < 0, a negative demand (the whole call fails).  FIT_E_STATE: before fit_load_nodes; while a
 * timeline is loaded; on a context created with world > 1 or FIT_FLAG_COLLECTIVES.  Three bounded
 * launches, no persistent grid: neither the per-GPU persistent-launch lock nor the watchdog. */
int fit_room(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
             const int32_t* wall, const uint16_t* part, struct fit_room* out);
/* Same with device pointers (inputs resident in HBM, the rows written in HBM; out 8-byte aligned). */
int fit_room_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                    const int32_t* wall, const uint16_t* part, struct fit_room* out);
/* Diagnostic, for measurement only (tools/room_bench.py): device time of the last successful
 * fit_room_device on this context, in milliseconds (HIP events on the context's own stream around
 * its launches).  FIT_E_STATE when there has been none. */
int fit_room_ms(fit_ctx* ctx, double* ms);
/* The row as one line of text, NUL-terminated into buf.  Host only: no device, no context.
 * Returns the length written (without the NUL), or FIT_E_INVAL: NULL arguments, an unknown code,
 * or a buffer too small for the text and its NUL (256 bytes always suffice).  The exact texts,
 * <x> a decimal field of the row:
 *   FIT_ROOM_SOME       "room for <copies> more on <nodes>/<members> nodes (at most <best> on one
 *                        node): limited by gpu on <by_gpu>, cpu on <by_cpu>, memory on <by_mem>"
 *                       — on one line, terms joined by ", "; a term whose count is 0 is left out,
 *                       and with no term left the ": limited by " goes too
 *     with best == FIT_ROOM_UNBOUNDED instead
 *                       "no resource demand: unlimited room on <nodes>/<members> nodes"
 *   FIT_ROOM_NONE       "no room now on any of <members> nodes"
 *   FIT_ROOM_NO_NODES / LIMIT_TIME / LIMIT_CPUS / LIMIT_MEM / PARTITION: fit_why_message's texts of
 *                       the codes with the same numbers, verbatim */
int fit_room_message(const struct fit_room* r, char* buf, int32_t buflen);

/* ---- which running jobs to evict so that a pending job fits -----------------
 * The other half of kube-scheduler's answer for a pod that does not fit: its PostFilter plugin
 * DefaultPreemption, Slurm's PreemptType=preempt/partition_prio — "evict these two jobs on node 812
 * and it runs now".  It needs one piece of state beside the node table: the preemptible running jobs
 * of every node.
 *
 * fit_load_victims: a CSR by the caller's node id, as fit_load_timeline's release events: node x's
 * victims are the entries [vic_off[x], vic_off[x+1]), each a running job's priority (any int32) and
 * what it holds on that node (cpus, MiB, GPUs, each >= 0).  Within a node the entries are in
 * EVICTION ORDER: priority non-decreasing, the lowest first; among equal priorities the caller's
 * order is kept.  vic_off has n + 1 entries; vic_off NULL = every list is empty.  Host pointers.
 * Call after fit_load_nodes, which drops the victims (node ids change); fit_place and the timeline
 * calls leave them alone.  Victims of a node in no partition are validated and never used.
 * FIT_E_INVAL: NULL ctx; vic_off[0] != 0 or a decreasing vic_off; a NULL column when there are
 * entries; a negative amount; priorities that decrease inside a node.  The call then fails as a
 * whole and the victims loaded before stay in place.  FIT_E_STATE: before fit_load_nodes; on a
 * context created with world > 1 or FIT_FLAG_COLLECTIVES. */
int fit_load_victims(fit_ctx* ctx, const int32_t* vic_off /* n + 1 */, const int32_t* vic_prio,
                     const int32_t* vic_cpu, const int32_t* vic_mem, const int32_t* vic_gpu);
/* Same with device pointers, validated by a kernel; n_vic = vic_off[n] (the caller knows it; a
 * vic_off that does not end there is FIT_E_INVAL, as is n_vic < 0 or n_vic > 0 with a NULL array). */
int fit_load_victims_device(fit_ctx* ctx, const int32_t* vic_off, int64_t n_vic, const int32_t* vic_prio,
                            const int32_t* vic_cpu, const int32_t* vic_mem, const int32_t* vic_gpu);

/* fit_preempt judges each of J one-node jobs ALONE against the context's current node table — the
 * rows fit_read_nodes returns, with the loaded avail_min / part_mask — and the loaded victims, and
 * changes nothing, as fit_explain does.  prio[j] is the job's priority (any int32).
 *   Node n is ELIGIBLE for a job when the job's partition bit is set in its mask, avail_min >= wall
 *   and all three free columns are >= 0 (a column loaded negative closes the node, as in
 *   fit_free_tl: the engine's row holds max(value, -1), no exact sum starts from that).
 *   L(n)   = the number of n's victims with priority STRICTLY BELOW the job's: a prefix of its list.
 *   S_c(v) = the exact sum of column c over the first v entries of n's list (64 bits).
 *   v(n)   = the smallest v in [0, L(n)] with free_c + S_c(v) >= demand_c in all three columns.
 *            v(n) = 0: the node fits now, exactly fit_explain's four terms.
 * The node: with fit > 0 the smallest (score of free - demand, node id) among the nodes that fit
 * now — what a fit_place of this job alone returns; victims = top_prio = 0.  Else with able > 0 the
 * smallest key (top, v, score, node id): top the priority of entry v - 1, the highest-priority job
 * evicted (kube-scheduler's first criterion), then fewer victims, then score, DESIGN §2's score of
 * min(free_c + S_c(v), INT32_MAX) - demand_c; the caller evicts the entries [vic_off[node],
 * vic_off[node] + victims) and the job fits node.  Else node = -1, victims = top_prio = 0.  One
 * 32-byte row per job.  Not judged here: multi-node jobs, sparing a victim of the prefix that turns
 * out not to be needed (the last one always is), the timeline. */
#define FIT_PRE_FITS 0        /* fit > 0: no eviction needed                                      */
#define FIT_PRE_PARTITION 1   /* = FIT_WHY_PARTITION    these four: FIT_WHY_*'s numbers, rule and */
#define FIT_PRE_LIMIT_TIME 2  /* = FIT_WHY_LIMIT_TIME   order; every other field is 0, with       */
#define FIT_PRE_LIMIT_CPUS 3  /* = FIT_WHY_LIMIT_CPUS   node = -1                                 */
#define FIT_PRE_LIMIT_MEM 4   /* = FIT_WHY_LIMIT_MEM                                              */
#define FIT_PRE_NO_NODES 5    /* members == 0 (= FIT_WHY_NO_NODES)                                */
#define FIT_PRE_EVICT 6       /* fit == 0, able > 0                                               */
#define FIT_PRE_NONE 7        /* fit == 0, able == 0                                              */
/* Precedence: 1, 2, 3, 4, 5, 0, 6, 7 (first match wins). */
typedef struct {              /* 32 bytes                                                         */
    int32_t code;        /* FIT_PRE_*                                                             */
    int32_t node;        /* the chosen node id, -1 if none                                        */
    int32_t victims;     /* entries of node's list to evict, from its first; 0 unless EVICT       */
    int32_t top_prio;    /* priority of the last of them, the highest evicted; 0 unless EVICT     */
    int32_t members;     /* nodes with the job's partition bit set (= fit_why.members)            */
    int32_t fit;         /* eligible nodes with v = 0 (= fit_why.fit at nodes_k 1)                */
    int32_t able;        /* eligible nodes with v >= 1                                            */
    int32_t outranked;   /* eligible nodes with no v in [0, L] where some v in (L, list length]   */
                         /* would do: jobs of equal or higher priority hold them                  */
} fit_evict;
/* Host pointers.  j == 0 returns 0 whatever the pointers are.  FIT_E_INVAL: NULL ctx / arrays,
 * j < 0, a negative cpu / mem / gpu / wall (the whole call fails).  FIT_E_STATE: before
 * fit_load_nodes; before any fit_load_victims since; while a timeline is loaded; on a context
 * created with world > 1 or FIT_FLAG_COLLECTIVES.  Bounded launches (three per 16,384 jobs), no
 * persistent grid: neither the per-GPU persistent-launch lock nor the watchdog. */
int fit_preempt(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                const int32_t* wall, const uint16_t* part, const int32_t* prio, fit_evict* out);
/* Same with device pointers (inputs resident in HBM, the rows written in HBM). */
int fit_preempt_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                       const int32_t* wall, const uint16_t* part, const int32_t* prio, fit_evict* out);
/* Diagnostic, for measurement only (tools/preempt_bench.py): device time of the last successful
 * fit_preempt_device on this context, in milliseconds (HIP events on the context's own stream
 * around its launches).  FIT_E_STATE when there has been none. */
int fit_preempt_ms(fit_ctx* ctx, double* ms);
/* The row as one line of text, NUL-terminated into buf.  Host only: no device, no context.
 * Returns the length written (without the NUL), or FIT_E_INVAL: NULL arguments, an unknown code,
 * or a buffer too small for the text and its NUL (256 bytes always suffice).  The exact texts,
 * <x> a decimal field of the row:
 *   FIT_PRE_FITS        "<fit>/<members> nodes fit now"
 *   FIT_PRE_EVICT       "fits node <node> after evicting <victims> lower-priority jobs (highest
 *                        priority <top_prio>): <able>/<members> nodes can be freed" — on one line
 *   FIT_PRE_NONE        "no node can be freed on any of <members> nodes: <outranked> held by jobs of
 *                        equal or higher priority" — on one line; with outranked == 0 the colon and
 *                       everything after it are left out
 *   FIT_PRE_NO_NODES / LIMIT_TIME / LIMIT_CPUS / LIMIT_MEM / PARTITION: fit_why_message's texts of
 *                       the codes with the same numbers, verbatim */
int fit_preempt_message(const fit_evict* r, char* buf, int32_t buflen);

/* ---- which victims to evict so that a MULTI-NODE job fits -------------------
 * fit_preempt for a job that needs need = max(nodes_k, 1) distinct nodes at once, 1 <= need <= kmax
 * <= FIT_MAX_K: Slurm's preempt/partition_prio for a wide job.  State, eligibility, L(n), S_c(v),
 * v(n) and the counters members / fit / able / outranked are fit_preempt's, unchanged; each job is
 * judged alone and nothing is written.  Every eligible node with some v(n) in [0, L(n)] has
 * fit_preempt's key (top, v, score, node id); a node that fits now (v = 0) has first word 0 and sorts
 * before every node that needs an eviction.  The keys are distinct (the node id is in them).  A job
 * has picks when fit + able >= need: the `need` smallest keys, in key order.  So every fitting node is
 * taken before any eviction, the highest evicted priority is the smallest possible for `need` nodes,
 * then fewer victims win, then the better fit, then the lower node id.
 *   out_node[q * kmax + i], i < need: the picks in key order;
 *   out_victims[q * kmax + i]: the pick's v, 0 for a node that fits now — the caller evicts the
 *     entries [vic_off[node], vic_off[node] + v) of each pick;
 *   every other entry is -1 in out_node and 0 in out_victims: i >= need, and every row whose code is
 *     neither FITS nor EVICT.
 * The codes are FIT_PRE_* with fit_preempt's precedence (1, 2, 3, 4, 5, 0, 6, 7):
 *   FIT_PRE_FITS   fit >= need            FIT_PRE_EVICT  fit < need <= fit + able
 *   FIT_PRE_NONE   fit + able < need (members < need included)      FIT_PRE_NO_NODES  members == 0
 * For codes 1-4 every field but code and need is 0.  With need == 1 the row and entry 0 of the two
 * arrays are fit_preempt's row, field for field.  Not judged here: sparing a victim of a prefix, the
 * timeline, the admitter; nothing is evicted. */
typedef struct {              /* 40 bytes                                                         */
    int32_t code;        /* FIT_PRE_*                                                             */
    int32_t need;        /* max(nodes_k, 1); set for every code                                   */
    int32_t evict_nodes; /* picks with v >= 1                                                     */
    int32_t victims;     /* the sum of the picks' v (exact: distinct nodes of an int32 CSR)       */
    int32_t top_prio;    /* the highest priority evicted: the last pick's top; 0 if evict_nodes 0 */
    int32_t members;     /* as fit_evict                                                          */
    int32_t fit;
    int32_t able;
    int32_t outranked;
    int32_t reserved;    /* 0                                                                     */
} fit_evict_k;
/* Host pointers; nodes_k NULL = every job needs one node.  j == 0 returns 0 whatever the pointers
 * are.  FIT_E_INVAL: NULL ctx / arrays, j < 0, kmax outside [1, FIT_MAX_K], a max(nodes_k, 1) above
 * kmax, a negative cpu / mem / gpu / wall (the whole call fails).  FIT_E_STATE: as fit_preempt.
 * Bounded launches (three per 16,384 jobs), no persistent grid: neither the per-GPU
 * persistent-launch lock nor the watchdog. */
int fit_preempt_k(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                  const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k /* NULL = all 1 */,
                  const int32_t* prio, int32_t kmax, fit_evict_k* out, int32_t* out_node /* j*kmax */,
                  int32_t* out_victims /* j*kmax */);
/* Same with device pointers (inputs resident in HBM, the rows and the picks written in HBM). */
int fit_preempt_k_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                         const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, const int32_t* prio,
                         int32_t kmax, fit_evict_k* out, int32_t* out_node, int32_t* out_victims);
/* Diagnostic, for measurement only (tools/preempt_k_bench.py): device time of the last successful
 * fit_preempt_k_device on this context, in milliseconds.  FIT_E_STATE when there has been none. */
int fit_preempt_k_ms(fit_ctx* ctx, double* ms);
/* The row as one line of text; return value and errors as fit_room_message's (256 bytes always
 * suffice).  The exact texts, <x> a decimal field of the row:
 *   FIT_PRE_FITS        "fits now on <need> of <fit>/<members> nodes"
 *   FIT_PRE_EVICT       "fits <need> nodes after evicting <victims> lower-priority jobs on
 *                        <evict_nodes> of them (highest priority <top_prio>): <fit> fit now, <able> can
 *                        be freed, of <members> nodes" — on one line
 *   FIT_PRE_NONE        "needs <need> nodes: <fit> fit now, <able> can be freed, of <members> nodes:
 *                        <outranked> held by jobs of equal or higher priority" — on one line; with
 *                       outranked == 0 the last colon and everything after it are left out
 *   FIT_PRE_NO_NODES / LIMIT_TIME / LIMIT_CPUS / LIMIT_MEM / PARTITION: fit_why_message's texts of
 *                       the codes with the same numbers, verbatim */
int fit_preempt_k_message(const fit_evict_k* r, char* buf, int32_t buflen);

/* ---- which running jobs to evict so that a job starts now ON THE TIMELINE ----
 * fit_preempt for a caller who keeps the loaded timeline: the node table does not see the
 * reservations that backfill committed, and a victim that ends at slot 3 frees nothing at slot 5,
 * where a reservation of a higher-priority pending job sits.
 *
 * fit_load_victims_tl: fit_load_victims' CSR with one more column.  vic_end[k] is the slot at which
 * the running job hands its resources back anyway (its release slot in fit_load_timeline's release
 * events), 0 <= end <= H, H the loaded horizon.  Evicting the entry adds its amounts to the slots
 * [0, end) of its node — what fit_unplace_tl with start 0 and wall end * slot_min does; an entry
 * with end 0 frees nothing and keeps its place in the list.  vic_off NULL = every list is empty.
 * These lists are independent of fit_load_victims': fit_load_nodes and fit_load_timeline drop them,
 * fit_place_tl(_k), fit_unplace_tl and fit_hold_tl leave them alone, and fit_advance_tl(a) keeps them:
 * from then on every end reads as max(end - a, 0) (the shifts add up, at most H; a new
 * fit_load_victims_tl starts from 0 again).  FIT_E_INVAL: fit_load_victims' list, or an end outside
 * [0, H]; the call then fails as a whole and the lists loaded before stay in place.  FIT_E_STATE:
 * before fit_load_nodes; without a timeline; on a context created with world > 1 or
 * FIT_FLAG_COLLECTIVES. */
int fit_load_victims_tl(fit_ctx* ctx, const int32_t* vic_off /* n + 1 */, const int32_t* vic_prio,
                        const int32_t* vic_end, const int32_t* vic_cpu, const int32_t* vic_mem,
                        const int32_t* vic_gpu);
/* Same with device pointers, validated by a kernel; n_vic as fit_load_victims_device's. */
int fit_load_victims_tl_device(fit_ctx* ctx, const int32_t* vic_off, int64_t n_vic, const int32_t* vic_prio,
                               const int32_t* vic_end, const int32_t* vic_cpu, const int32_t* vic_mem,
                               const int32_t* vic_gpu);

/* fit_preempt_tl judges each of J one-node jobs ALONE against the current timeline — what
 * fit_read_timeline returns, reservations included — and the lists of fit_load_victims_tl, for a
 * start NOW: the window [0, d), d = max(1, ceil(wall / slot_min)).  Nothing is written.  The rows,
 * the codes with their precedence and fit_preempt_message are fit_preempt's; what changes is the
 * rule per node:
 *   Node n is ELIGIBLE when the job's partition bit is set in its mask, d <= H and every slot of
 *   [0, d) reads >= 0 in all three columns (a -1 slot is closed and no eviction opens it).
 *   L(n)      = the number of n's entries with priority STRICTLY BELOW the job's.
 *   E_c(v, t) = the exact sum of column c over those of the first v entries whose end is > t.
 *   v(n)      = the smallest v in [0, L(n)] with free_c(n, t) + E_c(v, t) >= demand_c for every t in
 *               [0, d) and every column c.
 * members, fit (v = 0), able (v >= 1) and outranked (no v in [0, L], some v in (L, list length]) count
 * the nodes as fit_preempt does.  The node: with fit > 0 the smallest (score, node id) among the
 * fitting nodes, the score of the window minima minus the demand — fit_when's node; victims =
 * top_prio = 0.  Else with able > 0 the smallest (top, v, score, node id), top the priority of entry
 * v - 1 and score that of min over t in [0, d) of min(free_c(t) + E_c(v, t), INT32_MAX) - demand_c.
 * Else node = -1.  Not judged here: multi-node jobs, a start later than slot 0, sparing a victim of
 * the prefix; nothing is evicted.
 * Host pointers.  j == 0 returns 0 whatever the pointers are.  FIT_E_INVAL: as fit_preempt.
 * FIT_E_STATE: before fit_load_nodes; without a timeline; before any fit_load_victims_tl since the
 * timeline was loaded; on a context created with world > 1 or FIT_FLAG_COLLECTIVES.  Bounded
 * launches (three per 16,384 jobs), no persistent grid: neither the per-GPU persistent-launch lock
 * nor the watchdog. */
int fit_preempt_tl(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                   const int32_t* wall, const uint16_t* part, const int32_t* prio, fit_evict* out);
/* Same with device pointers (inputs resident in HBM, the rows written in HBM). */
int fit_preempt_tl_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                          const int32_t* wall, const uint16_t* part, const int32_t* prio, fit_evict* out);
/* Diagnostic, for measurement only (tools/preempt_tl_bench.py): device time of the last successful
 * fit_preempt_tl_device on this context, in milliseconds.  FIT_E_STATE when there has been none. */
int fit_preempt_tl_ms(fit_ctx* ctx, double* ms);

/* ---- victims for a MULTI-NODE job on the timeline ----------------------------
 * fit_preempt_tl for a job that needs need = max(nodes_k, 1) distinct nodes at once, 1 <= need <= kmax
 * <= FIT_MAX_K, all of them from slot 0: the common window is [0, d).  The state is fit_preempt_tl's,
 * unchanged — the loaded timeline, the lists of fit_load_victims_tl with their ends, the shift of
 * fit_advance_tl; the row, the codes with their precedence, the picks and the text are
 * fit_preempt_k's (fit_evict_k, fit_preempt_k_message).  Each job is judged alone and nothing is
 * written.  Per node, eligibility, L(n), E_c(v, t), v(n) and the counters are fit_preempt_tl's; every
 * eligible node with some v(n) in [0, L(n)] has the key (top, v, score, node id), the score that of
 * min over t in [0, d) of min(free_c(t) + E_c(v, t), INT32_MAX) - demand_c, and a node that fits now
 * (v = 0) first word 0.  A job has picks when fit + able >= need: the `need` smallest keys, in key
 * order, in out_node / out_victims as fit_preempt_k's — the caller evicts the first out_victims
 * entries of each pick's list.  With need == 1 the row and entry 0 of the two arrays are
 * fit_preempt_tl's row, field for field; a FITS row lists the nodes fit_when_k lists.
 * Host pointers; nodes_k NULL = every job needs one node.  j == 0 returns 0 once the state and kmax
 * have been judged.  FIT_E_INVAL: as fit_preempt_k.  FIT_E_STATE: as fit_preempt_tl.  Bounded launches
 * (three per 16,384 jobs), no persistent grid: neither the per-GPU persistent-launch lock nor the
 * watchdog. */
int fit_preempt_tl_k(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                     const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k /* NULL = all 1 */,
                     const int32_t* prio, int32_t kmax, fit_evict_k* out, int32_t* out_node /* j*kmax */,
                     int32_t* out_victims /* j*kmax */);
/* Same with device pointers (inputs resident in HBM, the rows and the picks written in HBM). */
int fit_preempt_tl_k_device(fit_ctx* ctx, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                            const int32_t* wall, const uint16_t* part, const uint16_t* nodes_k, const int32_t* prio,
                            int32_t kmax, fit_evict_k* out, int32_t* out_node, int32_t* out_victims);
/* Diagnostic, for measurement only (tools/preempt_tl_k_bench.py): device time of the last successful
 * fit_preempt_tl_k_device on this context, in milliseconds.  FIT_E_STATE when there has been none. */
int fit_preempt_tl_k_ms(fit_ctx* ctx, double* ms);

/* ---- report evicted victims: off the lists, onto the timeline ----------------
 * The engine evicts nothing; a caller that HAS evicted (deleted the pods) says so here, and the
 * loaded timeline, the lists and the shift stay loaded: ask (fit_preempt_tl_k), delete the pods,
 * report (fit_evicted_tl), place (fit_place_tl_k starts the job at slot 0 on the freed nodes).
 * Row i says that entry pos[i] of node[i]'s list is gone: node[i] is the caller's node id, pos[i]
 * the position in that node's CURRENT list, 0 being the entry fit_preempt_tl would evict first.
 * Every position of a call refers to the lists as they are before the call; rows come in any order
 * and several may name one node.  With e' = max(end - shift, 0), the end the queries read, each
 * row's entry (prio, end, cpu, mem, gpu)
 *   - adds its amounts to the slots [0, e') of its node with fit_unplace_tl's arithmetic, column by
 *     column: a -1 stays -1, any other value rises and saturates at INT32_MAX (e' = 0: nothing);
 *   - leaves its list; the node's other entries keep their order.  The shift is unchanged.
 * Afterwards the context answers every call exactly as one that had received fit_unplace_tl of one
 * row per evicted entry with e' > 0 (its amounts, wall e' * slot_min, nodes_k 1, its node, start 0)
 * and then fit_load_victims_tl of the remaining entries with every end written as e'.
 * A node in no partition has no list (its loaded entries were validated and never used): both calls
 * below read it as empty, so a row that names it is a position out of range.
 * Host pointers.  FIT_E_INVAL: NULL ctx; m < 0; NULL node or pos with m > 0; a node id outside
 * [0, n); a position outside [0, current length of that node's list); the same (node, pos) pair
 * twice in one call.  The call then fails as a whole: everything is judged before anything is
 * written, the timeline and the lists read back byte-identical.  FIT_E_STATE: as fit_preempt_tl.
 * m == 0 returns 0 once the state has been judged.  A HIP error in the write phase drops the
 * timeline and the lists (fit_load_timeline, fit_load_victims_tl).  Bounded launches, no persistent
 * grid: neither the per-GPU persistent-launch lock nor the watchdog. */
int fit_evicted_tl(fit_ctx* ctx, int32_t m, const int32_t* node /* m */, const int32_t* pos /* m */);
/* Same with device pointers; the rows are judged by a kernel. */
int fit_evicted_tl_device(fit_ctx* ctx, int32_t m, const int32_t* node, const int32_t* pos);
/* Device time (HIP events) of the last successful fit_evicted_tl / fit_evicted_tl_device with m > 0,
 * as fit_unplace_tl_ms; FIT_E_STATE before the first. */
int fit_evicted_tl_ms(fit_ctx* ctx, double* ms);
/* The current lists as a CSR by the caller's node id: what a caller mirrors.  Reading changes
 * nothing.  off (n + 1 entries) is always written; the five columns only when all are non-NULL and
 * cap >= off[n], ends as e' and entries in list order — a first call with cap 0 and NULL columns
 * sizes the second.  Loading the result into a context with the same timeline gives the same answers
 * from every query.  FIT_E_INVAL: NULL ctx or off.  FIT_E_STATE: as fit_evicted_tl. */
int fit_read_victims_tl(fit_ctx* ctx, int32_t* off /* n + 1 */, int64_t cap, int32_t* prio, int32_t* end,
                        int32_t* cpu, int32_t* mem, int32_t* gpu);

/* ---- a node changes outside the plan: overwrite windows of the timeline -------
 * A node goes DOWN or DRAIN, comes back, gets a maintenance window, has its avail_min shortened or
 * lengthened or is reconfigured with other totals: the loaded timeline, the victims' lists and their
 * shift stay loaded, and the caller writes the node's new levels here.  Let T be the dense timeline
 * fit_read_timeline returns and H the loaded horizon.  A row with from[q] < 0 is SKIPPED whatever else
 * it holds.  A live row covers the slots [from[q], min(to[q], H)) of node[q] (the caller's node id;
 * to = INT32_MAX: to the horizon) and gives each column its level cpu[q], mem[q], gpu[q] >= -1,
 * independently: -1 closes the column, a row may close one column only.  The result is that of the
 * live rows applied one after another in index order:
 *   T'[n][t][c] = the level of the live row with the LARGEST index that covers (n, t); T[n][t][c]
 *   where none does.
 * So one call equals any split of its rows into consecutive calls, a call repeated gives what one
 * gives, and rows on different nodes or disjoint windows commute.  A resumed node is a base row
 * [0, H) followed by the rows of its pending releases — the runs of its target timeline.
 * A node that was in no partition at fit_load_nodes has no run list: a live row naming it is valid,
 * writes nothing (the node reads -1 as before) and counts in *ignored; *applied counts the live rows
 * whose node has a list.  Load a node that may come back with its partition bits and avail_min 0.
 * Run lists stay canonical, cnt, head[] and the three ceilings of every touched node are exact
 * afterwards, so every query and placement answers as on a timeline loaded dense-equal.  The node
 * table (fit_read_nodes), H, slot_min, the partitions and the fit_load_victims_tl lists with their
 * shift are untouched.  With the other writers: a column closed through slot H - 1 stays closed
 * under every fit_advance_tl (§2i) until a row reopens slot H - 1; fit_unplace_tl and fit_evicted_tl
 * add nothing to a closed slot, so reopen first, then hand back; fit_hold_tl refuses a row over a
 * closed slot.
 * Host pointers; applied and ignored may be NULL and are written on success only.  FIT_E_INVAL:
 * NULL ctx; m < 0; a NULL array with m > 0; in a live row a node id outside [0, n), from >= H,
 * to <= from or a level below -1.  The call then fails as a whole: the batch is judged before the
 * first write, the timeline and every header byte stay as they were.  m == 0 returns 0 once the state
 * has been judged, whatever the pointers are.  FIT_E_STATE: before fit_load_nodes; without a
 * timeline; on a context with world > 1 or FIT_FLAG_COLLECTIVES.  A HIP error in the write phase
 * drops the timeline (fit_load_timeline).  Bounded launches (four kernels per 16,384 rows), no persistent
 * grid: neither the per-GPU persistent-launch lock nor the watchdog. */
int fit_set_tl(fit_ctx* ctx, int32_t m, const int32_t* node /* m */, const int32_t* from /* m */,
               const int32_t* to /* m */, const int32_t* cpu /* m */, const int32_t* mem /* m */,
               const int32_t* gpu /* m */, int64_t* applied /* may be NULL */, int64_t* ignored /* may be NULL */);
/* Same with the six columns as device pointers (applied and ignored stay host pointers); the rows are
 * judged by a kernel. */
int fit_set_tl_device(fit_ctx* ctx, int32_t m, const int32_t* node, const int32_t* from, const int32_t* to,
                      const int32_t* cpu, const int32_t* mem, const int32_t* gpu, int64_t* applied, int64_t* ignored);
/* Device time (HIP events) of the last successful fit_set_tl / fit_set_tl_device with a live row, as
 * fit_unplace_tl_ms; FIT_E_STATE before the first. */
int fit_set_tl_ms(fit_ctx* ctx, double* ms);

/* ---- free capacity of every partition at every timeline slot ---------------
 * The per-partition answer while a timeline is loaded — how many GPUs partition p has free in two
 * hours, how many nodes are open at slot t, the largest one-node job that could run then — reduced
 * on the GPU from the run lists, without the dense read-back of fit_read_timeline.  Let T be the
 * dense timeline fit_read_timeline returns, H the loaded horizon and mask[n] the loaded partition
 * mask.  Slot (n, t) is OPEN iff T[n][t][c] >= 0 in all three columns; so a slot past the node's
 * avail_min, a node in no partition and a slot with a column loaded negative are closed: the
 * feasibility view of fit_place_tl and fit_hold_tl (such a slot takes no job, a zero demand
 * included).  Row p * H + t describes, for partition p < parts and slot t < H, the nodes n with bit
 * p of mask[n] set and (n, t) open.  `parts` (1..32) is the caller's choice and independent of
 * fit_load_partitions: membership is the mask bit, as in fit_partition_free; mask bits >= parts are
 * ignored, and a node in several partitions counts in each of them.  With no open member every
 * field is 0 and the maxima are -1.  Read-only: the timeline, its headers and the node table are
 * untouched, and two calls give the same bytes.  While a timeline is loaded fit_partition_free does
 * not see the reservations the timeline writers made (they leave the node table untouched): row
 * p * H + 0 is the capacity now. */
typedef struct {             /* 40 bytes, 8-byte aligned                                           */
    int64_t cpu, mem, gpu;   /* exact sums of T[n][t][c]; cannot overflow (2^29 nodes x 2^31)      */
    int32_t nodes;           /* open member nodes at slot t                                        */
    int32_t max_cpu, max_mem, max_gpu; /* column-wise maxima over them, -1 when nodes == 0.        */
                             /* Upper bounds: a one-node job with cpu > max_cpu cannot run at t;   */
                             /* the three maxima may come from different nodes                     */
} fit_free;
/* out: parts * H rows in host memory.  FIT_E_INVAL: NULL ctx or out, parts outside [1, 32].
 * FIT_E_STATE: before fit_load_nodes; without a timeline loaded; on a context created with
 * world > 1 or FIT_FLAG_COLLECTIVES.  A HIP error fails the call and leaves the timeline loaded:
 * nothing was written.  Three bounded launches, no persistent grid: neither the per-GPU
 * persistent-launch lock nor the watchdog. */
int fit_free_tl(fit_ctx* ctx, int32_t parts, fit_free* out /* parts * H rows, row p * H + t */);
/* Same with the rows written in HBM (out: device pointer, 8-byte aligned, else FIT_E_INVAL);
 * complete on return. */
int fit_free_tl_device(fit_ctx* ctx, int32_t parts, fit_free* out);
/* Device time (HIP events) of the last successful fit_free_tl / fit_free_tl_device, as
 * fit_advance_tl_ms; FIT_E_STATE before the first. */
int fit_free_tl_ms(fit_ctx* ctx, double* ms);
/* The row as one line of text, NUL-terminated into buf.  Host only: no device, no context.
 * Returns the length written (without the NUL), or FIT_E_INVAL: NULL arguments, or a buffer too
 * small for the text and its NUL (256 bytes always suffice).  The exact texts, <x> a decimal field
 * of the row:
 *   nodes > 0    "<nodes> nodes open: <cpu> cpus, <mem> MiB, <gpu> gpus free (at most <max_cpu> cpus,
 *                 <max_mem> MiB, <max_gpu> gpus on one node)" — on one line
 *   otherwise    "no open node" */
int fit_free_message(const fit_free* r, char* buf, int32_t buflen);

/* ---- ingest / demand helpers (host code, mirrors of the reference Go functions) -------- */
/* ParseDuration (pkg/slurm-agent/parse.go:36-109): 0 ok, FIT_E_UNLIMITED, FIT_E_PARSE. */
int fit_parse_duration(const char* s, int64_t* out_ns);

typedef struct {
    int64_t nodes, mem_per_node, cpu_per_node, wall_ns;
} fit_resources;
/* parseResources (parse.go:111-190). */
int fit_parse_resources(const char* text, fit_resources* out);

typedef struct {
    int64_t cpus, memory, gpus, allo_cpus, allo_memory, allo_gpus;
} fit_node;
/* Client.Nodes + parseNode (slurm.go:354-363, parse.go:291-308): parses `scontrol show nodes`
 * text into at most cap records; returns the record count or a negative code. */
int fit_parse_nodes(const char* text, fit_node* out, int32_t cap);
/* parsePartition (parse.go:278-289): NUL-separated node names into buf; returns count. */
int fit_parse_partition(const char* text, char* buf, int32_t buflen);
/* parsePartitionsNames (parse.go:192-210): NUL-separated names into buf; returns count. */
int fit_parse_partitions_names(const char* text, char* buf, int32_t buflen);

typedef struct {
    int64_t nodes, cpus_per_task, ntasks, ntasks_per_node, mem_per_cpu, wall_ns;
    char array[64];
} fit_job_resources;
/* extractBatchResourcesFromScript (pkg/slurm-bridge-operator/parse.go:30-69): FIT_E_PARSE where
 * the reference returns an error or panics (bare flag as the last #SBATCH token). */
int fit_extract_batch_resources(const char* script, fit_job_resources* out);
/* setRequireResourceBySpec + setDefaultRequireResource (pod.go:70-107). */
void fit_apply_spec(fit_job_resources* r, int64_t nodes, int64_t cpus_per_task,
                    int64_t mem_per_cpu, int64_t ntasks_per_node, const char* array,
                    int64_t ntasks);
/* parseArrayLen (parse.go:126-135). */
int64_t fit_array_len(const char* array);
/* genResourceListForPod (pod.go:143-162): the pod's cpu request and memory quantity (bytes). */
void fit_pod_request(const fit_job_resources* r, int64_t* cpu, int64_t* memory);
/* Engine demand vector for one (array task of a) job: DESIGN.md §2 "demand". */
int fit_job_demand(const fit_job_resources* r, int32_t* cpu, int32_t* mem_mib, int32_t* wall_min,
                   uint16_t* nodes_k);
/* GetPartitionCapacity (pkg/slurm-virtual-kubelet/node.go:169-199), reference arithmetic. */
void fit_partition_capacity(const fit_node* nodes, int32_t n, int64_t* cpu, int64_t* memory,
                            int64_t* gpu, int64_t* pods);

/* ---- node-table ingest -------------------------------------------------
 * `scontrol show nodes` text → the engine's node columns (fit_load_nodes order and meaning).
 * Records are split and CPUTot/CPUAlloc/RealMemory/AllocMem parsed exactly as Client.Nodes +
 * parseNode (slurm.go:354-363, parse.go:291-308); added: Gres/GresUsed gpu counts (gpu_free =
 * Gres − GresUsed; the reference never sets Gpus/AlloGpus), Partitions= → part_mask bit p for
 * the p-th name of `partitions` (np NUL-separated names), State (DOWN, DRAIN, FAIL, MAINT, '*'
 * not responding, ...) → part_mask 0 (never placed), NodeName → `names` (NUL-separated, may be
 * NULL).  avail_min = INT32_MAX.  Returns the record count, FIT_E_INVAL (cap / buffer too small),
 * FIT_E_PARSE (malformed gres count). */
int fit_ingest_nodes(const char* text, const char* partitions, int32_t np, int32_t cap,
                     int32_t* cpu_free, int32_t* mem_free, int32_t* gpu_free, int32_t* avail_min,
                     uint32_t* part_mask, char* names, int32_t names_len);
/* Slurm hostlist expansion ("node[01-03,7],gpu[1-2]-ib" → node01 node02 node03 node07 gpu1-ib
 * gpu2-ib), NUL-separated into buf; returns the count, FIT_E_PARSE or FIT_E_INVAL (buf too
 * small).  The fix for parsePartition's split of "Nodes=node[1-3,5]" (parse.go:278-289). */
int fit_expand_hostlist(const char* expr, char* buf, int32_t buflen);
/* The Partition RPC's node list (PartitionResponse.nodes, workload.proto; n NUL-separated entries
 * as parsePartition split them on every comma, parse.go:278-289: "node[1-3" "5]" for
 * "Nodes=node[1-3,5]") → the expanded node names, NUL-separated into buf, in hostlist order.
 * These are the names to send to the Nodes RPC (Client.Nodes, slurm.go:343-364, which joins them
 * with commas for `scontrol show nodes`); record i of its answer is name i, and a caller must
 * refuse the answer when the record count differs.  Returns the count, FIT_E_PARSE (malformed
 * hostlist, or a name listed twice), FIT_E_INVAL (buf too small: retry with a larger one). */
int fit_node_names(const char* entries, int32_t n, char* buf, int32_t buflen);

/* ---- batched admission (CreatePod's call site) -----------------
 * The virtual kubelet calls CreatePod(ctx, *v1.Pod) (pkg/slurm-virtual-kubelet/provider.go:35-60)
 * from 10 concurrent PodSyncWorkers (options/options.go:107), one pod per call; a non-nil error
 * makes the library retry the pod later.  A fit_admitter coalesces those calls: fit_admit blocks
 * while its request joins the open batch; the batch closes max_wait_us after its first request
 * (or at max_batch requests), is ordered by (priority, arrival), placed with ONE fit_place, and
 * every caller returns with its own result.  Placements consume the context's node table, so
 * later batches see them until the next fit_admitter_load_nodes (the node ticker,
 * provider.go:470-488).  All calls are thread-safe; while an admitter owns a context, use the
 * context only through it.  fit_admitter_destroy fails still-queued requests with FIT_E_STATE. */
typedef struct fit_admitter fit_admitter;
typedef struct {
    int64_t priority;  /* smaller first (e.g. pod creation time); ties keep arrival order   */
    int32_t cpu;       /* per-node demand as fit_job_demand derives it                      */
    int32_t mem_mib;
    int32_t gpu;
    int32_t wall_min;
    uint16_t part;     /* partition index (fit_load_partitions order)                       */
    uint16_t nodes_k;  /* --nodes, 0 = 1, <= FIT_MAX_K                                      */
    uint16_t flags;    /* FIT_REQ_*: set by fit_pod_demand                                   */
    uint16_t reserved;
} fit_admit_req;
/* fit_admit_req.flags: one task of an array job (an --array label or #SBATCH --array): its pod's
 * one sbatch serves every task, so fit_admitter_script never pins it to the task's nodes */
#define FIT_REQ_ARRAY 1
typedef struct {
    int32_t node[FIT_MAX_K]; /* node ids (nodes_k of them, rest -1), or node[0] = FIT_UNPLACED
                                (no capacity now: retry) / FIT_REJECTED (partition limits)  */
    int64_t batch;           /* batch sequence number (0, 1, ...)                           */
    int32_t batch_jobs;      /* requests placed together in that batch                      */
    int32_t order;           /* this request's index in the batch's placement order        */
    int64_t ticket;          /* reservation id (> 0) when placed, else 0: see "reservations" */
} fit_admit_res;
int fit_admitter_create(fit_ctx* ctx, int32_t max_batch, int32_t max_wait_us, fit_admitter** out);
/* Blocks until the request's batch is placed.  FIT_OK (result in *res), FIT_E_INVAL (bad
 * request: negative demand, nodes_k > FIT_MAX_K; not queued), FIT_E_STATE (admitter shutting
 * down / no node table), or the batch's fit_place error. */
int fit_admit(fit_admitter* a, const fit_admit_req* req, fit_admit_res* res);
/* All-or-nothing admission of n requests (the tasks of one array job, fit_pod_demand): they join
 * ONE batch, consecutively in arrival order at their own priority.  If any of them is not placed,
 * none is: every res[i].node[0] is FIT_REJECTED (some task violates the partition limits) or
 * FIT_UNPLACED, ticket 0, and the group takes nothing: the batch is placed again without it, so
 * every later request of the batch sees the table the group left untouched — the sequential
 * semantics of placing the requests one after the other (tests/test_callsite_gpu.py
 * test_groups_in_one_batch_match_oracle).  Errors as fit_admit. */
int fit_admit_group(fit_admitter* a, const fit_admit_req* reqs, int32_t n, fit_admit_res* res);
/* Replaces the node table between batches (the node ticker, provider.go:470-488).  Every open
 * reservation (admitted, neither confirmed nor released) is taken from the new table again
 * before it is loaded — Slurm does not count a job it has not allocated yet, so a refresh would
 * otherwise hand its capacity out twice. */
int fit_admitter_load_nodes(fit_admitter* a, int32_t n, const int32_t* cpu_free,
                            const int32_t* mem_free, const int32_t* gpu_free,
                            const int32_t* avail_min, const uint32_t* part_mask);
/* The same with the table's node names and provenance.  names (n NUL-separated, fit_node_names or
 * fit_ingest_nodes order; NULL = none): open reservations are carried over to the new table by
 * NAME, so a node added to or removed from the partition does not move them to another node, and
 * fit_admitter_script can pin a pod to its nodes.  flags FIT_TABLE_STATE: part_mask carries the
 * nodes' State (fit_ingest_nodes: a DOWN / DRAIN / powered-down node is in no partition), so the
 * engine never chooses a node slurmctld would refuse, and placements are pinned.  The gRPC Nodes
 * RPC's Node has no state (workload.proto:165-174): a table built from it marks a drained node
 * with free capacity schedulable, so by default its placements only gate capacity (the script is
 * not pinned); FIT_TABLE_PIN pins them anyway (the operator's choice: a pod pinned to a drained
 * node then pends in Slurm while its reservation holds the capacity, until a TTL or release).
 * generation: fit_admitter_generation() taken BEFORE the table was fetched (0 = now): a confirmed
 * reservation is dropped only by a table fetched after its confirmation (earlier tables do not
 * count the job yet), and a table older than the last one loaded is refused (FIT_E_STATE). */
#define FIT_TABLE_STATE 1
#define FIT_TABLE_PIN 2
typedef struct {
    int32_t n;
    const int32_t* cpu_free;
    const int32_t* mem_free;
    const int32_t* gpu_free;
    const int32_t* avail_min;
    const uint32_t* part_mask;
    const char* names;
    int32_t flags;
    int64_t generation;
} fit_node_table;
int fit_admitter_load_table(fit_admitter* a, const fit_node_table* t);
/* A new table generation (> every earlier one): take it before fetching a table from Slurm. */
int64_t fit_admitter_generation(fit_admitter* a);
/* The script to submit for one pod whose admission returned `tickets` (n of them): with
 * `#SBATCH --nodelist=<names>` (fit_script_with_nodelist) when the pod is one request (n == 1; an
 * array job's tasks share one sbatch and stay unpinned) and the ticket's nodes come from a named
 * table loaded with FIT_TABLE_STATE or FIT_TABLE_PIN; the script unchanged otherwise.  *pinned (may be NULL) = 1 when
 * the directive was added.  The names are those of the table the reservation lives in now, read
 * under the same lock as placements and reloads.  Returns the length written, FIT_E_INVAL (unknown
 * ticket, out too small: strlen(script) + 32 + Σ (strlen(name) + 1) suffices). */
int fit_admitter_script(fit_admitter* a, const int64_t* tickets, int32_t n, const char* script,
                        char* out, int32_t outlen, int32_t* pinned);
int fit_admitter_partition_free(fit_admitter* a, int32_t p, int64_t* cpu, int64_t* mem_mib,
                                int64_t* gpu);
/* Reservations.  A placed request holds its demand on its nodes from admission until:
 *   confirm — Slurm now counts the job (it is allocated: the agent's Nodes RPC includes it, e.g.
 *             the pod's job is RUNNING): the reservation is dropped at the next load, not
 *             re-applied (the table then carries the allocation);
 *   release — the job will not run (pod deleted, SubmitJob failed): its demand goes back to the
 *             current table before the next batch (requires a table loaded through
 *             fit_admitter_load_nodes, else FIT_E_STATE); a confirmed one is only forgotten;
 *   ttl     — fit_admitter_set_ttl(a, L), L > 0: an open reservation that L loads have
 *             re-applied is dropped (a lost confirmation cannot hold capacity forever; 0 = never).
 * FIT_E_INVAL: unknown ticket. */
int fit_admitter_confirm(fit_admitter* a, int64_t ticket);
int fit_admitter_release(fit_admitter* a, int64_t ticket);
int fit_admitter_set_ttl(fit_admitter* a, int32_t loads);
/* fit_explain of n requests against the admitter's table as the next batch would see it: the
 * engine's copy is first brought up to date the way a batch does it, so open reservations count
 * (a node whose last GPU is reserved shows in short_gpu) and a released one no longer does.
 * Thread-safe; it takes the lock that placements and loads take and does not queue behind the
 * coalescer, so it waits for at most the batch being placed.  priority and flags are ignored.
 * n == 0 returns 0.  Errors as fit_explain. */
int fit_admitter_explain(fit_admitter* a, const fit_admit_req* reqs, int32_t n, fit_why* out);
/* fit_room of n requests against the same table, brought up to date exactly as
 * fit_admitter_explain does; priority, flags and nodes_k are ignored.  n == 0 returns 0.  Errors
 * as fit_room. */
int fit_admitter_room(fit_admitter* a, const fit_admit_req* reqs, int32_t n, struct fit_room* out);
/* Open reservations / requests queued for the next batch (monitoring, tests). */
int fit_admitter_reservations(fit_admitter* a);
int fit_admitter_pending(fit_admitter* a);
void fit_admitter_destroy(fit_admitter* a);

/* ---- CreatePod call site -------------------------------------
 * What the virtual kubelet's CreatePod has in hand — the pod's sbo.kubecluster.org/<key> labels
 * (newSubmitRequestForPod, pkg/slurm-virtual-kubelet/provider.go:62-125; keys
 * pkg/common/labels.go:9-14) and its sbatch script (Containers[0].Command[0], provider.go:71) —
 * turned into engine requests, and the engine's decision written back into the script. */
typedef struct {
    const char* nodes;            /* sbo.kubecluster.org/nodes            (NULL = label absent) */
    const char* cpus_per_task;    /* sbo.kubecluster.org/cpus-per-task                          */
    const char* mem_per_cpu;      /* sbo.kubecluster.org/mem-per-cpu                            */
    const char* ntasks_per_node;  /* sbo.kubecluster.org/ntasks-per-node                        */
    const char* array;            /* sbo.kubecluster.org/array                                  */
    const char* ntasks;           /* sbo.kubecluster.org/ntask                                  */
} fit_pod_labels;
/* Slurm --array expression ("0-15", "1,3,5-7", "0-15:4", "1-100%10") → the number of distinct
 * task ids and how many may run at once (min(tasks, %limit)).  The fix of parseArrayLen
 * (pkg/slurm-bridge-operator/parse.go:126-135), which gives 0 for "1-10%2" and "1-3,5".
 * FIT_E_PARSE: malformed, or a task id above 4,194,303. */
int fit_array_tasks(const char* array, int64_t* tasks, int64_t* max_running);
/* Slurm's MaxArraySize (slurm.conf, default 1001: task ids 0 .. 1000), which fit_pod_demand
 * enforces as sbatch does.  1 <= n <= 4,194,304; returns the previous value or FIT_E_INVAL.
 * Process-wide. */
int32_t fit_set_max_array_size(int32_t n);
/* The pod's demand as sbatch sees it: the script's #SBATCH header (extractBatchResourcesFromScript,
 * parse.go:30-69: --time, --nodes, --mem-per-cpu, --cpus-per-task, --ntasks-per-node), overridden
 * by the labels (they reach sbatch as command-line flags, pkg/slurm-agent/slurm.go:189-229; a
 * value strconv.ParseInt rejects is skipped, as provider.go:74-123 logs and skips it), then the
 * operator's defaults (pod.go:97-107) and fit_job_demand's per-node rule.  An array job becomes
 * one request per task that may run at once (fit_array_tasks; each task runs on its own nodes).
 * Writes min(n, cap) requests (partition `part`, priority `priority`) and returns n >= 1, or
 * FIT_E_PARSE (malformed #SBATCH header or array) / FIT_E_INVAL (demand out of range, or an array
 * task id >= MaxArraySize: sbatch would refuse the job, fit_set_max_array_size). */
int fit_pod_demand(const fit_pod_labels* labels, const char* script, uint16_t part,
                   int64_t priority, fit_admit_req* out, int32_t cap);
/* The script with `#SBATCH --nodelist=<names of node[0..k)>` added as the last line of its
 * #SBATCH header (after the last header line, so it overrides an earlier --nodelist / -w and the
 * header stays contiguous for extractBatchResourcesFromScript), so slurmctld allocates the nodes
 * the engine reserved — SubmitJobRequest.script (workload.proto:66), no proto change.  names: the
 * node table's names, NUL-separated in node-id order (fit_ingest_nodes, or the Partition RPC's
 * list), n_names of them.  Returns the length written (NUL-terminated), FIT_E_INVAL (a node id
 * out of range, or out too small: it needs strlen(script) + 32 + Σ (strlen(name) + 1)). */
int fit_script_with_nodelist(const char* script, const char* names, int32_t n_names,
                             const int32_t* node, int32_t k, char* out, int32_t outlen);
/* ResourcesResponse (workload.proto:137-148, filled by pkg/slurm-agent/api/slurm.go:297-341:
 * wallTime in seconds, 0 when UNLIMITED; cpuPerNode / memPerNode, -1 or 0 when unlimited or
 * unset) → fit_load_partitions' limits (minutes rounded up, -1 = no limit). */
int fit_partition_limits(int64_t wall_time_s, int64_t cpu_per_node, int64_t mem_per_node,
                         int32_t* max_time_min, int32_t* max_cpus_per_node,
                         int32_t* max_mem_per_node);
/* NodesResponse rows (workload.proto:165-174, as fit_node) → fit_load_nodes columns: free =
 * total − alloc clamped to int32, avail_min = INT32_MAX, part_mask for every row. */
int fit_node_columns(const fit_node* nodes, int32_t n, uint32_t part_mask, int32_t* cpu_free,
                     int32_t* mem_free, int32_t* gpu_free, int32_t* avail_min,
                     uint32_t* mask);

#ifdef __cplusplus
}
#endif
#endif /* FITGPU_H */

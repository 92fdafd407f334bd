// fit_device.h — data layouts shared by the HIP kernels and the host engine.
#pragma once
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <stdint.h>

namespace fitgpu {

#ifndef FIT_KS
#define FIT_KS 16
#endif
constexpr int KS = FIT_KS;      // candidates kept per (job, block-slice) by fit_scan
// the per-wave insertion network and the LDS bitonic merge tree of k_scan need a power of two
// (a FIT_KS=12 build placed jobs wrongly before this check)
// k_engine's workers dispatch on the per-component key count with cases 16, 8, 4 and 2 only
// (fit_persistent.hip): a larger FIT_KS would have no case
static_assert(KS >= 2 && KS <= 16 && (KS & (KS - 1)) == 0, "FIT_KS must be a power of two in [2, 16]");
constexpr int SCAN_WAVES = 8;   // waves per scan block; each walks one sub-slice of nodes
constexpr int SCAN_JOBS = 64;   // jobs per scan block (lanes = jobs, shared by the 8 waves)
#ifndef FIT_MIN_SUB
#define FIT_MIN_SUB 64
#endif
constexpr int MIN_SUB = FIT_MIN_SUB;  // minimum nodes per wave sub-slice
#ifndef FIT_MAX_SLICES
#define FIT_MAX_SLICES (128 / FIT_KS)
#endif
constexpr int MAX_SLICES = FIT_MAX_SLICES;  // block-slices per job per rank (sub-slice grows past this)
#ifndef FIT_TL_KS
#define FIT_TL_KS 4
#endif
constexpr int TL_KS = FIT_TL_KS;  // candidates per (job, block-slice) of the backfill scan
static_assert(TL_KS >= 1 && TL_KS <= 64 && (TL_KS & (TL_KS - 1)) == 0, "FIT_TL_KS must be a power of two");
#ifndef FIT_UCAP
#define FIT_UCAP 128  // 256: fewer dirty-full stops, but 6 helper entries per lane instead of 4
#endif                 // (C3 k_engine 33.6 -> 32.3 ms at 128, C2 -4 %, C3o +2 %)
constexpr int UCAP = FIT_UCAP;       // dirty-node capacity per component per round (UCAP / 64 per lane)
constexpr int MAX_COMPONENT_NODES = 1 << 20;  // LDS dirty bitmap limit (128 KiB)
constexpr uint64_t KEY_INF = ~0ull;
constexpr int FIT_KMAX = 8;     // nodes per multi-node job (include/fitgpu.h FIT_MAX_K)

// One Slurm node row in HBM, 32 B: read by fit_scan with one scalar s_load_dwordx8.
struct alignas(32) NodeRec {
    int32_t cpu, mem, gpu, avail;  // free cpus, free MiB, free GPUs, availability horizon (min)
    uint32_t mask;                 // partition membership bits
    int32_t orig;                  // node id in the caller's order (Client.Nodes order)
    int32_t pad0, pad1;
};

// Job row of the current window, written by fit_scan (slice 0), read by fit_commit.
struct alignas(32) JobRec {
    int32_t q;        // job index in the caller's priority order
    int32_t cpu, mem, gpu, wall;
    uint32_t pbit;    // 1u << partition
    int32_t k;        // nodes per job
    int32_t pad;
};

// Per-component plan for one round (host-built, uploaded each round).
struct alignas(16) CompPlan {
    int32_t nb, ne;      // component's node positions [nb, ne)
    int32_t sb, se;      // this rank's scan range inside it
    int32_t nslice;      // block-slices per job on every rank (<= MAX_SLICES)
    int32_t sub;         // nodes per wave sub-slice (block-slice = SCAN_WAVES * sub)
    int32_t jbase;       // first window job's index into the component job list
    int32_t w;           // window size (jobs)
    int32_t blk0;        // first fit_scan block of this component
    int32_t ks;          // keys kept per (job, block-slice): KS, or fewer for a large component
    int64_t cand_off;    // u64 offset of the component's candidates inside one rank section
    int32_t slot0;       // first window slot (global over components)
    int32_t k0;          // persistent engines, the round's first job tile: bit 0 keeps FIT_K0 keys
                         // (k_engine, k = 1 window); bit 1 scans it as paired half-slices (*_T0PAIR);
                         // bit 2 keeps FIT_K0W keys, unpaired (k_engine, after a first-tile rescan)
    int32_t pair_off;    // u64 offset of the round's half-slice list scratch (bit 1 of k0)
};

// Persistent engine (fit_persistent.hip): per-component state written by the host, results
// written by the component's committer wave.
struct CompState {
    int32_t nb, ne, sb, se, nslice, sub;
    int32_t jstart, jend;  // component job list range
    int64_t cand_off;      // fixed candidate region of this component (even rounds)
    int32_t slot0;         // fixed window slot region (even rounds)
    int32_t wmin, wmax;
    int32_t ks;            // keys per (job, block-slice) (CompPlan::ks)
    int32_t onepart;       // 1: the component is exactly one partition — every node's mask and every
                           // job's pbit is that partition's bit (k_engine's slim ring)
    int64_t cand_alt;     // the same for odd rounds (fit_engine_ctl.h: two buffer sets by parity)
    int32_t slot_alt;
    int32_t pair_off;      // half-slice list scratch (even rounds; odd: + PAIR_AREA)
};

// Per-component minimum demands (k_prefilter → k_engine's committers, DESIGN.md §3.7 recycling):
// jmin[3 * k + {0, 1, 2}] = the smallest cpu / mem / gpu demand among component k's non-rejected
// jobs, preset to JMIN_FILL bytes (0x7f7f7f7f: a component without jobs) before the prefilter.
constexpr int ENGINE_MAXC = 32;   // components (one per partition at most)
constexpr int JMIN_FILL = 0x7f;   // memset byte of the preset
struct EngineCompIds {            // launch component i of the persistent engine = component id[i]
    int8_t id[ENGINE_MAXC];
};

struct CompOut {
    int64_t evals, placed, done_jobs, rounds, stops_rescan, stops_dirty;
    int64_t t_commit, t_wait;  // 100 MHz realtime ticks spent committing / waiting for scans
};

// ---- SPEC §2b time-windowed backfill (fit_timeline.hip) --------------------
#ifndef FIT_TL_SPLIT_DEF
#define FIT_TL_SPLIT_DEF 0  // k_engine_tl as two concurrent launches (committers / scan workers); env FIT_TL_SPLIT
#endif
constexpr int TL_MAX_SLOTS = 1024;  // horizon limit (slots); the C5 horizon
#ifndef TL_UCAP_DEF
#define TL_UCAP_DEF 64
#endif
constexpr int TL_UCAP = TL_UCAP_DEF;  // dirty nodes per component per round (TL_UCAP / 64 per lane)
#ifndef FIT_TL_CAND
#define FIT_TL_CAND 128
#endif
constexpr int TL_CAND = FIT_TL_CAND;  // candidates per job of the timeline scan (64 or 128)
static_assert((TL_CAND == 64 || TL_CAND == 128) && TL_CAND % TL_KS == 0, "FIT_TL_CAND: 64 or 128");
constexpr int TL_SLICES = TL_CAND / TL_KS;  // block-slices per job (over all ranks) in the timeline scan
// The persistent engines' paired first tile (K_T0PAIR, TL_T0PAIR): one half-slice list of up to 4
// keys per (job, pair) held until its partner half merges it, per component and round parity
constexpr int PAIR_AREA = SCAN_JOBS * 32 * 4;
static_assert(TL_KS <= 4, "pair scratch holds 4 keys per (job, pair)");
constexpr int TL_MIN_SUB = 16;      // minimum nodes per wave sub-slice in the timeline scan (C5: 32 block-slices;
                                    // 32 gave 25 slices, 100 candidates: 129.8 vs 127.1 ms, r03j)
constexpr int TL_POS_BITS = 22;     // key = start << 54 | score << 22 | position
constexpr uint32_t TL_POS_MASK = (1u << TL_POS_BITS) - 1u;

// One run of equal free resources on a node's timeline: slots [previous end, end).  A node's
// list is canonical (adjacent runs differ) and ends at the horizon; at most TL_MAX_SLOTS runs.
struct alignas(16) Seg {
    int32_t end, cpu, mem, gpu;
};

constexpr int TL_HEAD = 4;  // runs of each node copied into its header (the scan's common case)

// Per-node header of a run list, 96 B, contiguous over nodes (the scan streams it): run count,
// a ceiling of each column — at least the largest free value on the node's timeline, so a job
// whose demand exceeds it cannot fit the node now — partition mask, node id, and a copy of the
// first TL_HEAD runs.  The ceilings are exact as built; reservations only lower values, which
// leaves them upper bounds, fit_unplace_tl, which raises values, raises them along (k_utl_apply,
// DESIGN.md §2h), and fit_advance_tl recomputes them exactly (k_atl_move).
struct alignas(32) TlHdr {
    int32_t cnt, cpu, mem, gpu;
    uint32_t mask;
    int32_t orig;  // node id in the caller's order (so a new dirty node needs no perm[] load)
    int32_t pad[2];
    Seg head[TL_HEAD];
};

struct CommitResult {
    int32_t done;   // jobs resolved this round (prefix of the window)
    int32_t stop;   // 0 window exhausted, 1 candidate list ran out, 2 dirty set full
    int32_t dirty;  // distinct nodes touched
    int32_t placed;
};

// Component node offsets for the direct small placement (k_small): nb[c] .. nb[c + 1].
struct SmallComps {
    int32_t nb[33];
};

// A small batch carried in k_small's kernel arguments (fit_place: no copy to the device; the
// kernarg segment holds up to 4 KB, this is 2,560 B).
constexpr int SMALL_ARGJ = 128;
struct SmallBatch {
    int32_t cpu[SMALL_ARGJ], mem[SMALL_ARGJ], gpu[SMALL_ARGJ], wall[SMALL_ARGJ];
    uint16_t part[SMALL_ARGJ], nk[SMALL_ARGJ];
};

// ---- the job-side queries (fit_query.h, DESIGN.md §3.11 "The query frame") --------------------
// What the partition-limit rule (job_limit) says of a job.  Codes 1..4 of every query's row are
// these; engine.cpp pins each family to include/fitgpu.h.
enum LimitCode : int32_t { LIM_NONE = 0, LIM_PARTITION = 1, LIM_LIMIT_TIME = 2, LIM_LIMIT_CPUS = 3, LIM_LIMIT_MEM = 4 };

// ---- fit_explain (fit_explain.hip) ------------------------------------
// The codes of include/fitgpu.h FIT_WHY_* (engine.cpp asserts they agree).
enum ExplainCode : int32_t {
    EX_FITS = LIM_NONE,
    EX_PARTITION = LIM_PARTITION,
    EX_LIMIT_TIME = LIM_LIMIT_TIME,
    EX_LIMIT_CPUS = LIM_LIMIT_CPUS,
    EX_LIMIT_MEM = LIM_LIMIT_MEM,
    EX_NO_NODES = 5,
    EX_RESOURCES = 6,
};
// Component node offsets in a query kernel's arguments: nb[c] .. nb[c + 1], c < ncomp.
struct ExplainComps {
    int32_t nb[33];
    int32_t ncomp;
};
hipError_t launch_explain_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                   const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                   const uint16_t* jpart, const uint16_t* jk, int32_t nj, void* out, int8_t* jcomp,
                                   int32_t* bad);
hipError_t launch_explain(hipStream_t st, const NodeRec* rec, const ExplainComps& C, const int32_t* jcpu,
                          const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                          int32_t nj, const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices,
                          void* out);
int explain_slices(int32_t nj, int32_t maxn, int cus, int min_rows = 32);

// ---- fit_when (fit_when.hip) -------------------------------------------
// The codes of include/fitgpu.h FIT_ETA_* (engine.cpp asserts they agree); 5 is EX_NO_NODES.
enum EtaCode : int32_t {
    ETA_NOW = LIM_NONE,
    ETA_PARTITION = LIM_PARTITION,
    ETA_LIMIT_TIME = LIM_LIMIT_TIME,
    ETA_LIMIT_CPUS = LIM_LIMIT_CPUS,
    ETA_LIMIT_MEM = LIM_LIMIT_MEM,
    ETA_NO_NODES = 5,
    ETA_LATER = 6,
    ETA_HORIZON = 7,
    ETA_WINDOW = 8,  // fit_when_k_win only: no start inside the job's window (SPEC §2r)
};
hipError_t launch_when_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                const uint16_t* jpart, int32_t nj, int32_t slot_min, void* out, int8_t* jcomp,
                                int32_t* bad);
hipError_t launch_when(hipStream_t st, const TlHdr* hdr, const Seg* slab, const ExplainComps& C, int32_t H,
                       int32_t slot_min, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                       const uint16_t* jpart, int32_t nj, const int8_t* jcomp, const int32_t* jl,
                       const int32_t* live, int slices, void* out);

// ---- fit_when_k (fit_when_k.hip) ---------------------------------------
// The codes are EtaCode's.  Scratch per chunk of jobs: a difference array of H + 1 words per job
// (64 MiB at WHENK_CHUNK jobs and H = 1,024) and WHENK_KEYS keys per (job, node slice).
constexpr int WHENK_CHUNK = 16384;    // jobs per count / pick / nodes / final sequence
constexpr int WHENK_GROUP = 8;       // jobs per k_whenk_count workgroup: 8 difference arrays in LDS (32.8 KB)
constexpr int WHENK_KEYS = 8;         // keys a node slice hands on per job (= FIT_KMAX)
constexpr int WHENK_MAX_SLICES = 16;  // node slices per job: k_whenk_final merges slices * WHENK_KEYS keys per job
hipError_t launch_whenk_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                 const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                 const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t nj,
                                 int32_t slot_min, void* out, int32_t* out_node, int8_t* jcomp, int32_t* bad);
hipError_t launch_whenk_chunk(hipStream_t st, const TlHdr* hdr, const Seg* slab, const ExplainComps& C, int32_t H,
                              int32_t slot_min, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                              const int32_t* jwall, const uint16_t* jpart, int32_t t0, int32_t nj, int32_t njobs,
                              int32_t kmax, const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices,
                              int32_t* diff, unsigned long long* top, void* out, int32_t* out_node);
// fit_when_k_win: the chunk with the windowed count, pick and final.  nb / dl:
// the job columns not_before and deadline on the device, either nullptr (all 0 / none).
hipError_t launch_whenk_chunk_win(hipStream_t st, const TlHdr* hdr, const Seg* slab, const ExplainComps& C, int32_t H,
                                  int32_t slot_min, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                                  const int32_t* jwall, const uint16_t* jpart, int32_t t0, int32_t nj, int32_t njobs,
                                  int32_t kmax, const int8_t* jcomp, const int32_t* jl, const int32_t* live,
                                  int slices, int32_t* diff, unsigned long long* top, void* out, int32_t* out_node,
                                  const int32_t* nb, const int32_t* dl);

// ---- fit_place_tl_k (fit_place_tl_k.hip) -------------------------------
// One workgroup per component walks its jobs in order; a launch takes at most PTLK_CHUNK jobs of
// every component's list, so a launch is bounded whatever J is.
constexpr int PTLK_CHUNK = 16384;   // jobs of a component per k_ptlk_commit launch
constexpr int PTLK_THREADS = 1024;  // threads of a commit workgroup, at most
hipError_t launch_ptlk_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t nj,
                                int32_t* out_node, int32_t* out_start, int8_t* jcomp);
int ptlk_threads(int32_t max_component_nodes);
size_t ptlk_lds_bytes(int threads, int32_t H);
hipError_t launch_ptlk_commit(hipStream_t st, int threads, TlHdr* hdr, Seg* slab, const ExplainComps& C, int32_t H,
                              int32_t slot_min, const int32_t* jl, const int32_t* jb, int32_t t0, int32_t chunk,
                              const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                              const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t* out_node,
                              int32_t* out_start, int32_t* placed);
// fit_place_tl_k_win: the windowed commit, nb / dl as launch_whenk_chunk_win's
hipError_t launch_ptlk_commit_win(hipStream_t st, int threads, TlHdr* hdr, Seg* slab, const ExplainComps& C, int32_t H,
                                  int32_t slot_min, const int32_t* jl, const int32_t* jb, int32_t t0, int32_t chunk,
                                  const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                  const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t* out_node,
                                  int32_t* out_start, int32_t* placed, const int32_t* nb, const int32_t* dl);

// ---- the rows of fit_unplace_tl and fit_hold_tl, grouped by node (fit_unplace_tl.hip, DESIGN.md
// §2h / §3.16) -----------------------------------------------------------------------------------
// Both calls take the same rows (demands, wall, nodes_k, node list, start), check the WHOLE batch
// with launch_utl_check, and group the windows of rows [t0, t0 + nj) by node with launch_utl_group:
// fit_unplace_tl per chunk of at most UTL_CHUNK rows, so a launch sequence is bounded whatever J is;
// fit_hold_tl once for the whole call (t0 = 0), since §2j judges per call.  The counter words g:
//   g[0]          touched nodes so far (k_utl_count)         } zero before every launch_utl_group
//   g[1]          windows handed out so far (k_utl_offsets)  }
//   g[2]          the bad-input flag (k_utl_check)
//   g[3]          pad (fit_set_tl: the live rows on a node without a run list, k_stl_check)
//   g[4 + chunk]  windows of that chunk's live rows (k_utl_check; chunk = row / the check's `chunk`)
constexpr int UTL_CHUNK = 16384;  // rows per launch sequence
// One window of one node, 32 B: two 16-byte loads (fit_tl_dense.h runs them over the dense columns)
struct alignas(16) TlWin {
    int32_t s, e;           // slots [s, e), clipped to the horizon
    int32_t cpu, mem, gpu;  // the demand handed back (fit_unplace_tl) or reserved (fit_hold_tl)
    int32_t row;            // its row: fit_hold_tl's windows set and obey the row's refused flag
    int32_t pad[2];
};
static_assert(sizeof(TlWin) == 32, "one window is two 16-byte loads");
hipError_t launch_utl_inverse(hipStream_t st, const TlHdr* hdr, int32_t nn, int32_t n, int32_t* inv);
hipError_t launch_utl_check(hipStream_t st, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                            const uint16_t* jk, int32_t kmax, const int32_t* node, const int32_t* start, int32_t nj,
                            int32_t n, int32_t H, int32_t chunk, int32_t* g);
// launch_utl_group's count and offsets alone (fit_set_tl scatters its own window format after them)
hipError_t launch_utl_ranges(hipStream_t st, int32_t nn, const uint16_t* jk, int32_t kmax, const int32_t* node,
                             const int32_t* start, int32_t t0, int32_t nj, int32_t windows, int32_t n,
                             const int32_t* inv, int32_t* cnt, int32_t* first, int32_t* fill, int32_t* touched,
                             int32_t* flag, int32_t* g);
// flag: null, or nj words: a row that names a node in no partition gets flag[row] = 1
hipError_t launch_utl_group(hipStream_t st, int32_t nn, int32_t H, int32_t slot_min, const int32_t* jcpu,
                            const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jk,
                            int32_t kmax, const int32_t* node, const int32_t* start, int32_t t0, int32_t nj,
                            int32_t windows, int32_t n, const int32_t* inv, int32_t* cnt, int32_t* first,
                            int32_t* fill, int32_t* touched, TlWin* win, int32_t* flag, int32_t* g);
hipError_t launch_utl_chunk(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t nn, int32_t H, int32_t slot_min,
                            const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                            const uint16_t* jk, int32_t kmax, const int32_t* node, const int32_t* start, int32_t t0,
                            int32_t nj, int32_t windows, int32_t n, const int32_t* inv, int32_t* cnt, int32_t* first,
                            int32_t* fill, int32_t* touched, TlWin* win, int32_t* g);

// ---- fit_advance_tl (fit_advance_tl.hip) -------------------------------
// Every node position's run list moved left by a slots, 1 <= a <= H, in place: one wave per list.
// *flag |= 1 when a tail entry of a caller's node id in [0, n) is below -1; nothing else is written
hipError_t launch_atl_check(hipStream_t st, const int32_t* tc, const int32_t* tm, const int32_t* tg, int32_t n,
                            int32_t* flag);
// tc / tm / tg: n entries in the caller's node order (TlHdr::orig indexes them), or all three null:
// every column continues its slot H - 1 value
hipError_t launch_atl_advance(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t nn, int32_t n, int32_t H, int32_t a,
                              const int32_t* tc, const int32_t* tm, const int32_t* tg);

// ---- fit_hold_tl (fit_hold_tl.hip) -------------------------------------
// The rows, their check, the node id -> position table and the grouping are the section above's.
hipError_t launch_htl_hold(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t nn, int32_t H, int32_t slot_min,
                           const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                           const uint16_t* jk, int32_t kmax, const int32_t* node, const int32_t* start, int32_t nj,
                           int32_t windows, int32_t n, const int32_t* inv, int32_t* cnt, int32_t* first,
                           int32_t* fill, int32_t* touched, TlWin* win, int32_t* flag, int32_t* g);
hipError_t launch_htl_final(hipStream_t st, const uint16_t* jk, int32_t kmax, const int32_t* start, int32_t nj,
                            const int32_t* flag, int32_t* out_state, unsigned long long* tot);

// ---- fit_free_tl (fit_free_tl.hip) -------------------------------------
// Read-only: per (partition, slot) the sums, node count and column maxima over the open member nodes.
constexpr int FREE_ROW_BYTES = 40;       // one fit_free row; the scratch planes take as much per row
// Node positions per k_free_walk workgroup.  The walk takes one header after the other, each a
// scalar load the next does not overlap, so its time goes with the chunk: at C5 0.27 ms at 64,
// 0.35 at 128, 0.65 at 256, 1.05 at 512
constexpr int FREE_CHUNK = 64;
constexpr int FREE_MAX_CHUNK = 1 << 16;  // the most FIT_FREE_CHUNK (measurements) may ask for
// scratch: FREE_ROW_BYTES * parts * H bytes; out: parts * H rows (row p * H + t); both 8-byte aligned
hipError_t launch_free_tl(hipStream_t st, const TlHdr* hdr, const Seg* slab, int32_t nn, int32_t H, int32_t parts,
                          int32_t chunk, void* scratch, void* out);

// ---- fit_room (fit_room.hip) -------------------------------------------
// The codes of include/fitgpu.h FIT_ROOM_* (engine.cpp asserts they agree); 5 is EX_NO_NODES.
enum RoomCode : int32_t {
    ROOM_SOME = LIM_NONE,
    ROOM_PARTITION = LIM_PARTITION,
    ROOM_LIMIT_TIME = LIM_LIMIT_TIME,
    ROOM_LIMIT_CPUS = LIM_LIMIT_CPUS,
    ROOM_LIMIT_MEM = LIM_LIMIT_MEM,
    ROOM_NO_NODES = 5,
    ROOM_NONE = 6,
};
hipError_t launch_room_classify(hipStream_t st, const int32_t* ptab, int32_t np, const int32_t* jcpu,
                                const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                                int32_t nj, void* out, int8_t* jcomp, int32_t* bad);
hipError_t launch_room(hipStream_t st, const NodeRec* rec, const ExplainComps& C, const int32_t* jcpu,
                       const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                       int32_t nj, const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices, void* out);

// ---- fit_load_victims / fit_preempt (fit_preempt.hip) -------------------
// The codes of include/fitgpu.h FIT_PRE_* (engine.cpp asserts they agree); 5 is EX_NO_NODES.
enum PreemptCode : int32_t {
    PRE_FITS = LIM_NONE,
    PRE_PARTITION = LIM_PARTITION,
    PRE_LIMIT_TIME = LIM_LIMIT_TIME,
    PRE_LIMIT_CPUS = LIM_LIMIT_CPUS,
    PRE_LIMIT_MEM = LIM_LIMIT_MEM,
    PRE_NO_NODES = 5,
    PRE_EVICT = 6,
    PRE_NONE = 7,
};
// One victim of a row, 16 B (one scalar s_load_dwordx4): its priority and the inclusive prefix sums
// of the row's amounts up to it, saturated at INT32_MAX
struct alignas(16) VicEnt {
    int32_t prio, cpu, mem, gpu;
};
constexpr int PRE_CHUNK = 16384;  // job positions per walk / final pair: the partials' bound
// the caller's CSR on the device: *bad |= 1 unless the offsets start at 0, do not decrease and end at
// nvic, the amounts are >= 0 and the priorities do not decrease inside a node
hipError_t launch_vic_check(hipStream_t st, const int32_t* off, int32_t n, int64_t nvic, const int32_t* prio,
                            const int32_t* cpu, const int32_t* mem, const int32_t* gpu, int32_t* bad);
// the checked CSR into row order: voff (nn + 1 row offsets, the caller's lists permuted) -> vent
hipError_t launch_vic_build(hipStream_t st, const int32_t* off, const int32_t* prio, const int32_t* cpu,
                            const int32_t* mem, const int32_t* gpu, const int32_t* perm, int32_t nn,
                            const int32_t* voff, VicEnt* vent);
hipError_t launch_preempt_classify(hipStream_t st, const int32_t* ptab, int32_t np, int ncomp, const int32_t* jcpu,
                                   const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                   const uint16_t* jpart, int32_t nj, void* out, int8_t* jcomp, int32_t* bad);
int preempt_slices(int32_t nj, int32_t maxn, int cus);
size_t preempt_partials(int32_t nj, int slices);  // 16-byte words of `part`
hipError_t launch_preempt(hipStream_t st, const NodeRec* rec, const int32_t* voff, const VicEnt* vent,
                          const ExplainComps& C, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                          const int32_t* jwall, const uint16_t* jpart, const int32_t* jprio, int32_t nj,
                          const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices, void* part,
                          void* out);

// ---- fit_preempt_k (fit_preempt_k.hip) ----------------------------------
// fit_preempt's codes, victims, slices and chunk; rows of 40 B (fit_evict_k), out_node / out_vic of
// nj * kmax entries, kmax in [1, FIT_KMAX]; *bad also for a nodes_k above kmax (jk nullptr: all 1)
hipError_t launch_preempt_k_classify(hipStream_t st, const int32_t* ptab, int32_t np, int ncomp, const int32_t* jcpu,
                                     const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                                     const uint16_t* jpart, const uint16_t* jk, int32_t kmax, int32_t nj, void* out,
                                     int32_t* out_node, int32_t* out_vic, int8_t* jcomp, int32_t* bad);
size_t preempt_k_partials(int32_t nj, int slices, int32_t kmax);  // 16-byte words of `part`
hipError_t launch_preempt_k(hipStream_t st, const NodeRec* rec, const int32_t* voff, const VicEnt* vent,
                            const ExplainComps& C, const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                            const int32_t* jwall, const uint16_t* jpart, const int32_t* jprio, int32_t kmax,
                            int32_t nj, const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices,
                            void* part, void* out, int32_t* out_node, int32_t* out_vic);

// ---- fit_load_victims_tl / fit_preempt_tl (fit_preempt_tl.hip) ---------
// fit_preempt's codes, rows, classifier, slices, chunk and partials; the walk reads the run lists.
// One victim of a node position, 32 B (one scalar s_load_dwordx8): its priority, the slot at which it
// hands its resources back anyway and the raw amounts it holds
struct alignas(32) VicTl {
    int32_t prio, end, cpu, mem, gpu, pad[3];  // pad[0]: fit_evicted_tl's mark, 0 outside that call
};
// The list of a node position: entries [beg, beg + len) of the entry array (one scalar 8-byte load).
// A pair per position, not shared offsets, so that fit_evicted_tl shrinks a list in place.
struct alignas(8) VicSpan {
    int32_t beg, len;
};
// launch_vic_check's test plus 0 <= end <= H
hipError_t launch_vtl_check(hipStream_t st, const int32_t* off, int32_t n, int64_t nvic, const int32_t* prio,
                            const int32_t* end, const int32_t* cpu, const int32_t* mem, const int32_t* gpu, int32_t H,
                            int32_t* bad);
hipError_t launch_vtl_build(hipStream_t st, const int32_t* off, const int32_t* prio, const int32_t* end,
                            const int32_t* cpu, const int32_t* mem, const int32_t* gpu, const int32_t* perm, int32_t nn,
                            const VicSpan* vspan, VicTl* vent);
// k_pre_final (fit_preempt.hip) for the positions [t0, t0 + nt) of a walk's partials
hipError_t launch_preempt_final(hipStream_t st, const int32_t* jl, const int32_t* live, int32_t nj, int32_t t0,
                                int32_t nt, int ncomp, int slices, const int8_t* jcomp, const void* part, void* out);
// shift: the slots fit_advance_tl has moved the timeline by since the victims were loaded, in [0, H]
hipError_t launch_preempt_tl(hipStream_t st, const TlHdr* hdr, const Seg* slab, const VicSpan* vspan, const VicTl* vent,
                             const ExplainComps& C, int32_t H, int32_t slot_min, int32_t shift, const int32_t* jcpu,
                             const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                             const int32_t* jprio, int32_t nj, const int8_t* jcomp, const int32_t* jl,
                             const int32_t* live, int slices, void* part, void* out);

// ---- fit_preempt_tl_k (fit_preempt_tl_k.hip) ----------------------------
// fit_preempt_tl's state and walk frame with fit_preempt_k's rows, classifier, lists and final kernel.
// k_prek_final (fit_preempt_k.hip) for the positions [t0, t0 + nt) of a walk's lists of kmax keys
hipError_t launch_preempt_k_final(hipStream_t st, const int32_t* jl, const int32_t* live, int32_t nj, int32_t t0,
                                  int32_t nt, int ncomp, int slices, int32_t kmax, const int8_t* jcomp,
                                  const void* part, void* out, int32_t* out_node, int32_t* out_vic);
hipError_t launch_preempt_tl_k(hipStream_t st, const TlHdr* hdr, const Seg* slab, const VicSpan* vspan,
                               const VicTl* vent, const ExplainComps& C, int32_t H, int32_t slot_min, int32_t shift,
                               const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                               const uint16_t* jpart, const int32_t* jprio, int32_t kmax, int32_t nj,
                               const int8_t* jcomp, const int32_t* jl, const int32_t* live, int slices, void* part,
                               void* out, int32_t* out_node, int32_t* out_vic);

// ---- fit_evicted_tl (fit_evicted_tl.hip) -------------------------------
// The caller's report of evicted entries: row q names entry pos[q] of node[q]'s list (caller's node
// id).  inv, cnt, touched and the counter words g are fit_unplace_tl's (g[0] touched nodes, g[2] the
// bad-input flag; cnt[nn] and g zero before the first check).  A check marks the entries of rows
// [t0, t0 + nj), nj <= UTL_CHUNK; clear takes the marks of a refused call back; apply, one wave per
// touched node, adds the marked entries' windows to the run list and compacts the victim list.
hipError_t launch_etl_check(hipStream_t st, const int32_t* node, const int32_t* pos, int32_t t0, int32_t nj, int32_t n,
                            const int32_t* inv, const VicSpan* vspan, VicTl* vent, int32_t* cnt, int32_t* touched,
                            int32_t cap, int32_t* g);
hipError_t launch_etl_clear(hipStream_t st, const int32_t* node, const int32_t* pos, int32_t nj, int32_t n,
                            const int32_t* inv, const VicSpan* vspan, VicTl* vent);
hipError_t launch_etl_apply(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t H, int32_t shift, const int32_t* touched,
                            int32_t cap, VicSpan* vspan, VicTl* vent, const int32_t* g);

// ---- fit_set_tl (fit_set_tl.hip) ---------------------------------------
// Rows (node, from, to, cpu, mem, gpu) that overwrite windows of the loaded timeline; the row with
// the largest index stands where rows overlap.  inv, cnt, first, fill, touched, win and the counter
// words g are fit_unplace_tl's, with g[3] the live rows whose node has no run list (ignored) and
// g[4 + chunk] the rows of that chunk whose node has one (its windows).  The check judges the WHOLE
// batch (inv complete before it); a chunk is rows [t0, t0 + nj), nj <= UTL_CHUNK: count and offsets
// (launch_utl_ranges), the scatter and the apply, one wave per touched node over four dense columns.
hipError_t launch_stl_check(hipStream_t st, const int32_t* node, const int32_t* from, const int32_t* to,
                            const int32_t* cpu, const int32_t* mem, const int32_t* gpu, int32_t m, int32_t n, int32_t H,
                            int32_t chunk, const int32_t* inv, int32_t* g);
hipError_t launch_stl_chunk(hipStream_t st, TlHdr* hdr, Seg* slab, int32_t nn, int32_t H, const int32_t* node,
                            const int32_t* from, const int32_t* to, const int32_t* cpu, const int32_t* mem,
                            const int32_t* gpu, int32_t t0, int32_t nj, int32_t windows, int32_t n, const int32_t* inv,
                            int32_t* cnt, int32_t* first, int32_t* fill, int32_t* touched, TlWin* win, int32_t* g);

// Persistent engines' watchdog trip record (fit_engine_ctl.h; read back by engine.cpp).
enum TripSite : unsigned {
    TRIP_NONE = 0,
    TRIP_WORKER_RING = 1,   // scan worker: its claimed ring slot got no task (arg = ring index)
    TRIP_ROUND_START = 2,   // committer: tiles of the round before last not done (arg = target)
    TRIP_HELPER_TILE = 3,   // commit helper: a job tile's scan not done (arg = tile)
    TRIP_HELPER_SNAP = 4,   // commit helper: the decider did not advance (arg = record)
    TRIP_DECIDER_REC = 5,   // decider: a helper record not ready (arg = record)
    TRIP_SINGLE_TILE = 6,   // single-wave commit: a job tile's scan not done (arg = tile)
    TRIP_NO_PROGRESS = 7,   // a round resolved no job
    TRIP_NO_KERNEL = 8,     // no scan kernel for the plan's key count
    TRIP_PEER = 9,          // drained after another block's trip
};
struct TripRec {  // the launch's first trip (claim 0 -> 1); plain stores, read after the kernel
    unsigned claim, site, comp, round;
    unsigned arg, q_head, q_tail, pubt;
    unsigned tdone, need, block, pad;
    unsigned long long waited;  // realtime ticks (10 ns) the wait lasted
    unsigned long long when;    // realtime at the trip, minus the launch's start stamp
};


// ---- launch functions and sizing queries of the .hip files, as the host engine calls them ------
hipError_t launch_scan(int blocks, hipStream_t st, const NodeRec* rec, const int32_t* jl,
                       const int32_t* jcpu, const int32_t* jmem, const int32_t* jgpu,
                       const int32_t* jwall, const uint16_t* jpart, const uint16_t* jk,
                       const CompPlan* plan, int ncomp, uint64_t* cand, uint64_t* bnd,
                       JobRec* wjob);
hipError_t launch_commit(int ncomp, int epl, size_t lds_bytes, hipStream_t st, NodeRec* rec,
                         const CompPlan* plan, const uint64_t* cand, int64_t rank_stride,
                         int nranks, const uint64_t* bnd, const JobRec* wjob, int32_t* out,
                         int kmax, CommitResult* res);
hipError_t launch_prefilter(hipStream_t st, const int32_t* jcpu, const int32_t* jmem,
                            const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart, const uint16_t* jk,
                            int32_t nj, int32_t kmax, const int32_t* ptab, int32_t np,
                            int32_t* out, int8_t* jcomp, int32_t* jmin = nullptr);
size_t joblists_scratch_ints(int32_t nj);
hipError_t launch_joblists(hipStream_t st, const int8_t* jcomp, int32_t nj, int ncomp,
                           int32_t* scratch, int32_t* g, int32_t* jb, int32_t* mb, int32_t* jl,
                           int32_t* jpk);
hipError_t launch_small_args(hipStream_t st, int ncomp, NodeRec* rec, const SmallComps& C, const int32_t* ptab,
                             int32_t np, const SmallBatch& B, bool has_nk, int32_t nj, int32_t kmax, int32_t* out,
                             int32_t* stat);
hipError_t launch_small(hipStream_t st, int ncomp, NodeRec* rec, const SmallComps& C,
                        const int32_t* ptab, int32_t np, const int32_t* jcpu, const int32_t* jmem,
                        const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                        const uint16_t* jk, int32_t nj, int32_t kmax, int32_t* out, int32_t* stat);
hipError_t launch_gather_nodes(hipStream_t st, const int32_t* cpu, const int32_t* mem,
                               const int32_t* gpu, const int32_t* av, const uint32_t* mask,
                               const int32_t* perm, int32_t nn, NodeRec* rec);
hipError_t launch_scatter_nodes(hipStream_t st, const NodeRec* rec, int32_t nn, int32_t* cpu,
                                int32_t* mem, int32_t* gpu);
size_t engine_lds_bytes(int32_t max_component_nodes);
// demand-class engine (fit_class.hip)
size_t class_lds_bytes(int32_t max_component_nodes);
int class_max();
int class_table_slots();
size_t class_slot_bytes();
int class_max_nodes();
hipError_t launch_classify(hipStream_t st, const int8_t* jcomp, const int32_t* jcpu, const int32_t* jmem,
                           const int32_t* jgpu, const uint16_t* jpart, int32_t nj, void* tab, int4* dem,
                           int32_t* ncls, int16_t* jcls);
hipError_t launch_class(hipStream_t st, int ncomp, size_t lds, NodeRec* rec, const int32_t* nbv, uint32_t owned,
                        const int32_t* jb, const int32_t* jl, const int32_t* jwall, const uint16_t* jk,
                        const int16_t* jcls, const int4* dem, const int32_t* ncls, int32_t kmax, int32_t* out,
                        CompOut* co, unsigned* err);
hipError_t launch_class_out(hipStream_t st, int32_t* out, int64_t n, const NodeRec* rec);
size_t engine_ctl_bytes();
size_t engine_ctl_error_offset();
size_t engine_ctl_trip_offset();
size_t engine_ring_bytes();
size_t engine_ring_tasks();
int engine_ring_groups();
int engine_blocks_per_cu(size_t lds);
hipError_t launch_engine(int blocks, size_t lds, hipStream_t st, void* ctl, void* ring,
                         const void* cs, void* co, CompPlan* plans, int ncomp, NodeRec* rec,
                         const int32_t* jl, const int32_t* jcpu, const int32_t* jmem,
                         const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                         const uint16_t* jk, uint64_t* cand, uint64_t* bnd, JobRec* wjob,
                         int32_t* out, int kmax, int64_t* wbusy, const int32_t* jpk, unsigned wd,
                         const int32_t* jmin, const EngineCompIds& ids);
// time-windowed backfill (fit_timeline.hip)
hipError_t launch_build_tl(hipStream_t st, const int32_t* cpu, const int32_t* mem,
                           const int32_t* gpu, const int32_t* av, const uint32_t* mask,
                           const int32_t* perm, int32_t nn, int32_t H, int32_t slot_min,
                           const int32_t* off, const int32_t* rs, const int32_t* rc,
                           const int32_t* rm, const int32_t* rg, Seg* slab, TlHdr* hdr,
                           uint32_t* err);
hipError_t launch_scan_tl(int blocks, hipStream_t st, const Seg* slab, const TlHdr* hdr,
                          const int32_t* jl, const int32_t* jcpu, const int32_t* jmem,
                          const int32_t* jgpu, const int32_t* jwall, const uint16_t* jpart,
                          const CompPlan* plan, int ncomp, uint64_t* cand, uint64_t* bnd,
                          JobRec* wjob, int32_t H, int32_t slot_min);
size_t commit_tl_lds_bytes(int32_t max_component_nodes);
int commit_tl_runs(int32_t max_component_nodes);
hipError_t launch_commit_tl(int ncomp, int epl, size_t lds, hipStream_t st, Seg* slab,
                            TlHdr* hdr, const CompPlan* plan, const uint64_t* cand,
                            int64_t rank_stride, int nranks, const uint64_t* bnd,
                            const JobRec* wjob, const int32_t* perm, int32_t* out, int32_t* outs,
                            CommitResult* res, int32_t H, int32_t R);
int engine_tl_runs(int32_t max_component_nodes);
size_t engine_tl_lds_bytes(int32_t max_component_nodes);
int engine_tl_blocks_per_cu(size_t lds, int mode);
size_t engine_tl_scan_lds_bytes();
hipError_t launch_engine_tl(int blocks, size_t lds, hipStream_t st, void* ctl, void* ring,
                            const void* cs, void* co, CompPlan* plans, int ncomp, Seg* slab,
                            TlHdr* hdr, const int32_t* jl, const int32_t* jcpu,
                            const int32_t* jmem, const int32_t* jgpu, const int32_t* jwall,
                            const uint16_t* jpart, uint64_t* cand, uint64_t* bnd, JobRec* wjob,
                            const int32_t* perm, int32_t* out, int32_t* outs, int32_t H,
                            int32_t slot_min, int32_t R, int64_t* wbusy, int mode,
                            unsigned* resident, unsigned wd);
hipError_t launch_expand_tl(hipStream_t st, const int32_t* perm, const Seg* slab,
                            const TlHdr* hdr, int32_t nn, int32_t H, int32_t* oc, int32_t* om,
                            int32_t* og);

}  // namespace fitgpu

// engine.cpp — host runtime of libfitgpu.so: context, node-table ingest into HBM, the
// speculative round loop, node sharding over RCCL.  DESIGN.md §3.
//
// Boundary: include/fitgpu.h.  Everything here is plain C++ over the HIP runtime; the compute
// is in fit_kernels.hip.  There is no CPU placement path: without a gfx950 device fit_create
// fails with FIT_E_NODEV.
#include <errno.h>
#include <fcntl.h>
#include <hip/hip_runtime_api.h>
#include <hip/hip_vector_types.h>
#include <rccl/rccl.h>
#include <sys/file.h>
#include <sys/stat.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <map>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/fitgpu.h"
#include "fit_device.h"

using namespace fitgpu;

namespace {

// components sharing the fullest task ring (fit_engine_ctl.h: component c goes to ring
// c % min(groups, nc))
inline int64_t ring_comps(int nc) {
    const int g = std::max(1, std::min(engine_ring_groups(), nc));
    return (nc + g - 1) / g;
}

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

#define HIP_TRY(expr)                                                                       \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(FIT_E_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_),   \
                        __FILE__, __LINE__);                                                \
    } while (0)

#define NCCL_TRY(expr)                                                                      \
    do {                                                                                    \
        ncclResult_t r_ = (expr);                                                           \
        if (r_ != ncclSuccess)                                                              \
            return fail(FIT_E_RCCL, "%s failed: %s", #expr, ncclGetErrorString(r_));        \
    } while (0)

// device buffer that only grows; owns its memory
template <class T>
struct DBuf {
    T* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return 0;
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(n, 64);
        if (hipMalloc(&p, want * sizeof(T)) != hipSuccess) {
            p = nullptr;
            return fail(FIT_E_OOM, "hipMalloc(%zu bytes) failed", want * sizeof(T));
        }
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    DBuf() = default;
    DBuf(const DBuf&) = delete;
    DBuf& operator=(const DBuf&) = delete;
    ~DBuf() { release(); }
};

template <class T>
struct HBuf {  // pinned host buffer
    T* p = nullptr;
    size_t cap = 0;
    int ensure(size_t n) {
        if (n <= cap) return 0;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        size_t want = std::max<size_t>(n, 64);
        if (hipHostMalloc(&p, want * sizeof(T), hipHostMallocDefault) != hipSuccess) {
            p = nullptr;
            return fail(FIT_E_OOM, "hipHostMalloc(%zu bytes) failed", want * sizeof(T));
        }
        cap = want;
        return 0;
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    HBuf() = default;
    HBuf(const HBuf&) = delete;
    HBuf& operator=(const HBuf&) = delete;
    ~HBuf() { release(); }
};

// fit_explain / fit_when: the rows on the device (host entry point; the flag word rides behind
// them), the flag word of the device entry point, the pinned copy both come back into, and the
// device time of the last *_device call (fit_explain_ms / fit_when_ms)
template <class Row>
struct QueryBufs {
    DBuf<Row> out;
    DBuf<int32_t> bad;
    HBuf<Row> h;
    double ms = -1;
};

int find_root(int* par, int x) {
    while (par[x] != x) x = par[x] = par[par[x]];
    return x;
}

double now_ms() {
    using namespace std::chrono;
    return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

// ---- per-device arbitration of persistent launches (round 5) --------------------------------
// A persistent launch (k_engine / k_engine_tl) needs its committer blocks resident while its scan
// workers spin on the task ring.  Alone on the GPU every block of its grid is resident (the grid
// is sized by occupancy).  Two side by side are not: the dispatcher hands each grid's blocks to
// the 8 XCDs in block order, so launch A's committer on XCD k can queue behind launch B's blocks
// while A's workers fill the other XCDs waiting for it — and B's committer waits behind A's
// workers (GPUTEST_r04: the watchdog tripped with three contexts on one GPU).  One virtual kubelet
// per partition (pkg/configurator/configurator.go:151-171) means several contexts per GPU, in
// several processes, so every persistent launch on a device is serialised: a process-wide mutex
// per device, then an exclusive flock on <FIT_LOCK_DIR or /tmp>/fitgpu-<PCI bus id>.lock for the
// other processes (flock: released by the kernel if the holder dies).  Held from the launch to
// the stream synchronisation that ends it.  The host-driven rounds (k_scan / k_commit, no
// cross-block waits) need no arbitration.
struct DevArb {
    std::mutex mu;
    int fd = -1;
    std::string path;
};

// The lock directory.  The lock only serialises launches whose processes see the same file, and
// the configurator runs every virtual kubelet as its own pod (configurator.go:188-293) with a
// private /tmp, so the default is a HOST path the VK pod template mounts:
//   FIT_LOCK_DIR if set (an explicit choice: used as given, a failure to open the file is an error);
//   else FIT_LOCK_DIR_DEFAULT when it is a directory (the hostPath volume, DirectoryOrCreate);
//   else /tmp — shared only inside one pod: returned as 1 so the caller can warn (fit_lock_dir).
constexpr const char* FIT_LOCK_DIR_DEFAULT = "/var/run/fitgpu";
int resolve_lock_dir(std::string& dir) {
    const char* e = getenv("FIT_LOCK_DIR");
    if (e && *e) {
        dir = e;
        return 0;
    }
    struct stat sb;
    if (stat(FIT_LOCK_DIR_DEFAULT, &sb) == 0 && S_ISDIR(sb.st_mode)) {
        dir = FIT_LOCK_DIR_DEFAULT;
        return 0;
    }
    dir = "/tmp";
    return 1;
}

DevArb* dev_arb(int device, std::string& err) {
    static std::mutex m;
    static std::map<int, DevArb*> tab;
    std::lock_guard<std::mutex> g(m);
    DevArb*& a = tab[device];
    if (!a) a = new DevArb();  // one per device for the process lifetime
    if (a->fd < 0) {
        char bus[64] = {0};
        if (hipDeviceGetPCIBusId(bus, sizeof bus, device) != hipSuccess) snprintf(bus, sizeof bus, "dev%d", device);
        for (char* q = bus; *q; ++q)
            if (*q == ':' || *q == '/') *q = '_';
        std::string dir;
        (void)resolve_lock_dir(dir);
        a->path = dir + "/fitgpu-" + bus + ".lock";
        // every user's engines share the file: created 0666 (fchmod, not the process-wide umask);
        // an existing file of another user in a sticky /tmp may refuse an O_CREAT open
        // (fs.protected_regular), so it is then opened read-only — flock needs no write access
        a->fd = open(a->path.c_str(), O_RDWR | O_CREAT | O_CLOEXEC, 0666);
        if (a->fd >= 0) (void)fchmod(a->fd, 0666);  // fails harmlessly on another user's file
        else a->fd = open(a->path.c_str(), O_RDONLY | O_CLOEXEC);
        if (a->fd < 0) {
            err = a->path + ": " + strerror(errno);
            return nullptr;
        }
    }
    return a;
}

struct ArbGuard {
    DevArb* a = nullptr;
    double waited_ms = 0;
    int take(int device) {
        const double t0 = now_ms();
        std::string err;
        DevArb* d = dev_arb(device, err);
        if (!d) return fail(FIT_E_STATE, "device lock %s (set FIT_LOCK_DIR to a writable directory)", err.c_str());
        d->mu.lock();
        int r;
        do r = flock(d->fd, LOCK_EX);
        while (r != 0 && errno == EINTR);
        if (r != 0) {
            d->mu.unlock();
            return fail(FIT_E_STATE, "flock %s: %s", d->path.c_str(), strerror(errno));
        }
        a = d;
        waited_ms = now_ms() - t0;
        return 0;
    }
    ~ArbGuard() {
        if (!a) return;
        (void)flock(a->fd, LOCK_UN);
        a->mu.unlock();
    }
};

}  // namespace

// The context's runtime handles.  A base of fit_ctx, so they go after every buffer member has
// freed its memory: events, the mapped flag, the streams, then the communicator.
struct CtxHandles {
    ncclComm_t comm = nullptr;
    hipStream_t st = nullptr;
    hipEvent_t ev[6] = {};
    // FIT_TL_SPLIT: the backfill engine's scan workers as a second, concurrent launch
    hipStream_t st2 = nullptr;
    hipEvent_t ev_join = nullptr;
    unsigned* resident = nullptr;  // host-mapped: committer blocks running
    CtxHandles() = default;
    CtxHandles(const CtxHandles&) = delete;
    CtxHandles& operator=(const CtxHandles&) = delete;
    ~CtxHandles() {
        for (auto& e : ev)
            if (e) (void)hipEventDestroy(e);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (resident) (void)hipHostFree(resident);
        if (st2) (void)hipStreamDestroy(st2);
        if (st) (void)hipStreamDestroy(st);
        if (comm) (void)ncclCommDestroy(comm);
    }
};

struct fit_ctx : CtxHandles {
    int device = 0;
    int rank = 0, world = 1;
    int shard_mode = FIT_SHARD_AUTO;
    fit_exchange_fn xchg = nullptr;  // host exchange instead of RCCL (tests, custom transport)
    void* xchg_user = nullptr;
    HBuf<uint8_t> h_x;               // staging for the host exchange
    DBuf<uint64_t> xcount;           // per-rank counters (component-sharded stats)
    bool force_coll = false;         // FIT_FLAG_COLLECTIVES: sharded path + exchange at world 1
    bool collective() const { return world > 1 || force_coll; }
    bool persistent = true;          // one-launch work-queue engine (FIT_ENGINE=rounds: host loop)
    // placements of at most this many jobs (after the partition-limit prefilter) run the
    // host-driven rounds instead of a whole-chip persistent grid: an admission batch of a few
    // hundred pods is one or two rounds of a few tiles (FIT_SMALL_BATCH)
    int32_t small_batch = 2048;
    // placements of at most this many jobs run k_small: one launch, the jobs one at a time against
    // every node of their component, no rounds and one host synchronisation (FIT_SMALL_DIRECT)
    // 128: where k_small stops beating the host-driven rounds on one VK's one-partition table
    // (tools/direct_vs_rounds.py, profiles/r06q_direct_vs_rounds.txt: 184 vs 178 µs at 128 jobs;
    // the 16-component C3 table breaks even near 1,024)
    int32_t small_direct = 128;
    // a batch of <= SMALL_ARGJ jobs from host memory rides in k_small's kernel arguments (no copy to
    // the device), and the call spins on the batch's completion event instead of sleeping in a
    // stream synchronisation (FIT_SMALL_ARGS=0 / FIT_SYNC_SPIN=0: A/B switches)
    bool small_args = true, sync_spin = true;
    // the demand-class engine (fit_class.hip): 0 off (FIT_CLASS=0, and FIT_ENGINE=persistent|rounds|
    // direct), 1 for placements the persistent engine would run (FIT_CLASS=1), 2 at every size
    // (FIT_ENGINE=class), 3 (the default) for those of them whose live jobs are at least half
    // multi-node; used when every component is one partition, fits LDS and has <= class_max()
    // demand classes
    int cls_mode = 3;
    int32_t last_multi = 0;          // multi-node jobs of the last job lists (build_job_lists)
    bool cls_nodes_ok = false;       // node table: single-partition components that fit LDS
    int32_t cls_maxn = 0;            // largest component (nodes)
    DBuf<int16_t> jcls;
    DBuf<uint8_t> cls_tab;
    DBuf<int4> cls_dem;
    DBuf<int32_t> cls_n;
    DBuf<unsigned> cls_err;
    HBuf<int32_t> h_cls_n;
    HBuf<unsigned> h_cls_err;
    DBuf<int32_t> small_placed;
    HBuf<int32_t> h_small;
    DBuf<uint8_t> jpack;    // fit_place's job columns of a small batch, packed: one H2D copy
    HBuf<uint8_t> h_jpack;
    // fit_explain / fit_when: the rows on the device, the device entry point's flag word, the
    // pinned copy and the *_ms diagnostic of each
    QueryBufs<fit_why> ex;
    QueryBufs<fit_eta> wh;
    QueryBufs<struct fit_room> rm;
    // fit_when_k: its rows, the node lists of the host entry point (device, pinned), and the
    // scratch of one job chunk — difference arrays and per-slice keys
    QueryBufs<fit_eta_k> wk;
    DBuf<int32_t> wk_node, wk_diff;
    HBuf<int32_t> h_wk_node;
    DBuf<unsigned long long> wk_top;
    // fit_when_k_win / fit_place_tl_k_win: the flag word, pinned copy and *_ms of the windowed query
    // (its rows' scratch is fit_when_k's), and the host entry points' staged window columns
    QueryBufs<fit_eta_k> wkw;
    DBuf<int32_t> win_nb, win_dl;
    // fit_place_tl_k: the placed count of the commit launches (device, pinned)
    DBuf<int32_t> ptlk_cnt;
    HBuf<int32_t> h_ptlk;
    // fit_unplace_tl and fit_hold_tl, ONE set between them: the staged node lists, starts and (hold)
    // states of the host entry points, node id -> position, per-position window count / range start /
    // scatter cursor, the touched positions and the windows of one grouping (a chunk of fit_unplace_tl,
    // the whole call of fit_hold_tl: each call sizes them), hold's per-row refused flags and two
    // 64-bit totals, the counter words (fit_device.h) and the pinned copies.
    // Sharing is safe: both calls run on the context's one stream and end synchronised, so the two
    // are never live at once, and each call clears or rebuilds every word it reads before it reads it.
    DBuf<int32_t> tlr_node, tlr_start, tlr_state, tlr_inv, tlr_cnt, tlr_first, tlr_fill, tlr_touched, tlr_flag, tlr_g;
    DBuf<TlWin> tlr_win;
    DBuf<unsigned long long> tlr_tot;
    HBuf<int32_t> h_tlr_g;
    HBuf<unsigned long long> h_tlr_tot;
    double utl_ms = -1, htl_ms = -1;  // the *_ms diagnostics of the two calls
    // fit_advance_tl: the staged tails of the host entry point, the bad-input flag with its pinned
    // copy, and the *_ms diagnostic
    DBuf<int32_t> atl_tc, atl_tm, atl_tg, atl_g;
    HBuf<int32_t> h_atl;
    double atl_ms = -1;
    // fit_free_tl: the accumulator planes, the rows of the host entry point and the *_ms diagnostic
    // 
    DBuf<int64_t> free_acc;
    DBuf<fit_free> free_rows;
    double free_ms = -1;
    // fit_load_victims / fit_preempt: the host entry point's staged CSR, the
    // check's flag word, the victims in row order (voff: nn + 1 offsets; vent: priority and saturated
    // prefix sums), then the query's rows, its staged priorities and the per-slice key partials
    DBuf<int32_t> vs_off, vs_prio, vs_cpu, vs_mem, vs_gpu, vic_bad, voff;
    HBuf<int32_t> h_vic_bad;
    DBuf<VicEnt> vent;
    bool have_vic = false;
    QueryBufs<fit_evict> pe;
    DBuf<int32_t> pe_prio;
    HBuf<int32_t> h_pe_prio;
    DBuf<uint4> pe_part;
    // fit_preempt_k: its rows and the picks of the host entry point (device,
    // pinned).  It shares fit_preempt's staged priorities and key scratch: both calls run on the
    // context's one stream and end synchronised, and each writes every word before it reads it.
    QueryBufs<fit_evict_k> pk;
    DBuf<int32_t> pk_node, pk_vic;
    HBuf<int32_t> h_pk_pick;
    // fit_load_victims_tl / fit_preempt_tl: the victims of the loaded timeline
    // in position order, their own buffers and flag (vtl_span: a (begin, length) pair per position;
    // vtl_ent: vtl_total entries of priority, end slot, raw amounts — fit_evicted_tl shortens a list in
    // place, so a span may cover less than it was loaded with), the slots fit_advance_tl has moved the
    // timeline by since they were loaded, and the query's rows.  The staged CSR (vs_*, vic_bad), the
    // staged priorities and the key scratch are fit_load_victims' and fit_preempt's: every call ends
    // synchronised on the one stream.
    DBuf<int32_t> vs_end;
    DBuf<VicSpan> vtl_span;
    DBuf<VicTl> vtl_ent;
    bool have_vtl = false;
    int32_t vtl_shift = 0, vtl_total = 0;
    // fit_evicted_tl: the staged rows of the host entry point and the *_ms
    // diagnostic; node id -> position, the counts, the touched list and the counter words are tlr_*'s
    DBuf<int32_t> etl_node, etl_pos;
    double etl_ms = -1;
    // fit_set_tl: the six staged columns of the host entry point, one after
    // another, and the *_ms diagnostic; everything else is tlr_*'s, under the rule stated there
    DBuf<int32_t> stl_rows;
    double stl_ms = -1;
    QueryBufs<fit_evict> pt;
    // fit_preempt_tl_k: its rows.  The victims and the shift are fit_preempt_tl's,
    // the staged priorities, the key scratch and the picks' buffers fit_preempt_k's.
    QueryBufs<fit_evict_k> ptk;
    int cus = 256;
    DBuf<uint8_t> ectl, ering;
    DBuf<CompState> ecs;
    DBuf<CompOut> eco;
    DBuf<int64_t> ebusy;
    HBuf<CompState> h_ecs;
    HBuf<CompOut> h_eco;
    HBuf<int64_t> h_ebusy;
    HBuf<uint32_t> h_err;
    HBuf<TripRec> h_trip;
    DBuf<NodeRec> rec_bak;           // node rows before a persistent launch (restored on a trip)
    unsigned wd_ticks = 1000000000u; // watchdog: realtime ticks (10 ns) a wait may last (10 s)
    HBuf<uint64_t> h_count;
    int wmin = 256, wmax = 8192;

    // node table
    int32_t n = 0;           // rows in caller order
    int32_t nn = 0;          // rows in components (mask != 0)
    int ncomp = 0;
    int comp_of_part[32];
    bool comp_onepart[32] = {false};  // the component is exactly one partition (CompState::onepart)
    std::vector<int32_t> nb;  // ncomp + 1 component offsets (positions)
    DBuf<NodeRec> rec;
    DBuf<int32_t> col_cpu, col_mem, col_gpu, col_av, perm;
    DBuf<uint32_t> col_mask;
    DBuf<int32_t> rb_cpu, rb_mem, rb_gpu;  // fit_read_nodes scratch (col_* stay the loaded table)
    std::vector<uint32_t> h_mask;
    std::vector<int32_t> h_perm;  // row position -> caller's node id (fit_load_victims orders its lists by it)
    bool have_nodes = false;
    int64_t loads = 0;        // successful node-table loads (admit.cpp notices a direct load)

    // partitions: [max_time | max_cpus | max_mem | comp] × 32
    int32_t np = 0;
    int32_t ptab[128];
    DBuf<int32_t> d_ptab;

    // per-call scratch
    DBuf<int32_t> jcpu, jmem, jgpu, jwall, out, jl, jpk;
    DBuf<uint16_t> jpart, jk;
    DBuf<int8_t> jcomp;
    DBuf<int32_t> jmin;  // per-component minimum demands of the placement's jobs (k_prefilter)
    DBuf<uint64_t> cand, bnd;
    DBuf<JobRec> wjob;
    DBuf<CompPlan> plan;
    DBuf<CommitResult> res;
    HBuf<CompPlan> h_plan;
    HBuf<CommitResult> h_res;
    DBuf<int32_t> jls;    // device job-list scratch (block counts, counters, offsets)
    HBuf<int32_t> h_jls;

    // time-windowed backfill: per-node run lists, built from the node
    // table + release events by fit_load_timeline
    int32_t tl_slots = 0, tl_slot_min = 0;
    bool have_tl = false;
    DBuf<Seg> slab;
    DBuf<TlHdr> tlhdr;
    DBuf<int32_t> outs, rel_off, rel_slot, rel_cpu, rel_mem, rel_gpu;
    DBuf<uint32_t> tl_err;
    HBuf<uint32_t> h_tl_err;
};

namespace {

int build_ptab(fit_ctx* c) {
    for (int p = 0; p < 32; ++p) c->ptab[96 + p] = c->comp_of_part[p];
    if (c->d_ptab.ensure(128)) return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->d_ptab.p, c->ptab, sizeof c->ptab, hipMemcpyHostToDevice, c->st));
    return 0;
}

// Components = partitions connected through nodes that belong to several of them; jobs of
// different components never compete for a node, so each is an independent sequence
// (DESIGN.md §3.1).  Nodes are laid out component by component, in id order inside each.
int load_nodes_common(fit_ctx* c, int32_t n) {
    int par[32];
    for (int i = 0; i < 32; ++i) par[i] = i;
    bool used[32] = {false};
    for (int32_t x = 0; x < n; ++x) {
        uint32_t m = c->h_mask[x];
        if (!m) continue;
        int lo = __builtin_ctz(m);
        for (uint32_t r = m; r; r &= r - 1) {
            int b = __builtin_ctz(r);
            used[b] = true;
            int ra = find_root(par, lo), rb = find_root(par, b);
            if (ra != rb) par[std::max(ra, rb)] = std::min(ra, rb);
        }
    }
    int root_comp[32];
    for (int i = 0; i < 32; ++i) root_comp[i] = -1;
    c->ncomp = 0;
    for (int p = 0; p < 32; ++p) {
        c->comp_of_part[p] = -1;
        if (!used[p]) continue;
        int r = find_root(par, p);
        if (root_comp[r] < 0) root_comp[r] = c->ncomp++;
        c->comp_of_part[p] = root_comp[r];
    }
    c->nb.assign(c->ncomp + 1, 0);
    for (int32_t x = 0; x < n; ++x)
        if (c->h_mask[x]) c->nb[c->comp_of_part[__builtin_ctz(c->h_mask[x])] + 1]++;
    for (int k = 0; k < c->ncomp; ++k) {
        if (c->nb[k + 1] > MAX_COMPONENT_NODES)
            return fail(FIT_E_INVAL, "partition component %d has %d nodes (limit %d)", k,
                        c->nb[k + 1], MAX_COMPONENT_NODES);
        c->nb[k + 1] += c->nb[k];
    }
    c->nn = c->nb[c->ncomp];
    {  // the class engine: one partition per component (the part test is then always true) and
       // the component's rows in one workgroup's LDS
        int parts_of[32] = {0};
        for (int p = 0; p < 32; ++p)
            if (c->comp_of_part[p] >= 0) ++parts_of[c->comp_of_part[p]];
        c->cls_nodes_ok = c->ncomp > 0 && c->ncomp <= 32;
        c->cls_maxn = 0;
        for (int k = 0; k < c->ncomp; ++k) {
            const int32_t nk = c->nb[k + 1] - c->nb[k];
            c->cls_maxn = std::max(c->cls_maxn, nk);
            if (parts_of[k] != 1) c->cls_nodes_ok = false;
        }
        for (int k = 0; k < 32; ++k) c->comp_onepart[k] = k < c->ncomp && parts_of[k] == 1;
        if (c->cls_maxn > class_max_nodes() || class_lds_bytes(c->cls_maxn) > 160 * 1024)
            c->cls_nodes_ok = false;
    }
    std::vector<int32_t> fill(c->nb.begin(), c->nb.end() - 1), perm(std::max(c->nn, 1));
    for (int32_t x = 0; x < n; ++x)
        if (c->h_mask[x]) perm[fill[c->comp_of_part[__builtin_ctz(c->h_mask[x])]]++] = x;
    if (c->perm.ensure(std::max(c->nn, 1)) || c->rec.ensure(std::max(c->nn, 1))) return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->perm.p, perm.data(), sizeof(int32_t) * c->nn, hipMemcpyHostToDevice,
                           c->st));
    HIP_TRY(launch_gather_nodes(c->st, c->col_cpu.p, c->col_mem.p, c->col_gpu.p, c->col_av.p,
                                c->col_mask.p, c->perm.p, c->nn, c->rec.p));
    int rc = build_ptab(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));
    perm.resize(c->nn);
    c->h_perm.swap(perm);
    c->n = n;
    c->have_nodes = true;
    c->have_tl = false;  // a timeline belongs to the node table it was built from
    ++c->loads;
    return 0;
}

int alloc_cols(fit_ctx* c, int32_t n) {
    size_t m = std::max<int32_t>(n, 1);
    if (c->col_cpu.ensure(m) || c->col_mem.ensure(m) || c->col_gpu.ensure(m) ||
        c->col_av.ensure(m) || c->col_mask.ensure(m))
        return FIT_E_OOM;
    return 0;
}

// ------------------------------------------------------------------------ exchange
// In-place collectives on device buffers: RCCL over xGMI, or the caller's host exchange.
int xchg(fit_ctx* c, int op, void* dbuf, int64_t count) {
    if (!c->collective() || count == 0) return 0;
    if (!c->xchg) {
        switch (op) {
            case FIT_XCHG_ALLGATHER_U64: {
                uint64_t* b = static_cast<uint64_t*>(dbuf);
                NCCL_TRY(ncclAllGather(b + (size_t)c->rank * count, b, count, ncclUint64, c->comm,
                                       c->st));
                return 0;
            }
            case FIT_XCHG_MIN_U64:
                NCCL_TRY(ncclAllReduce(dbuf, dbuf, count, ncclUint64, ncclMin, c->comm, c->st));
                return 0;
            case FIT_XCHG_MAX_I32:
                NCCL_TRY(ncclAllReduce(dbuf, dbuf, count, ncclInt32, ncclMax, c->comm, c->st));
                return 0;
            case FIT_XCHG_MIN_I32:
                NCCL_TRY(ncclAllReduce(dbuf, dbuf, count, ncclInt32, ncclMin, c->comm, c->st));
                return 0;
        }
        return fail(FIT_E_INVAL, "exchange op %d", op);
    }
    const size_t elem = (op == FIT_XCHG_ALLGATHER_U64 || op == FIT_XCHG_MIN_U64) ? 8 : 4;
    const size_t bytes = elem * (size_t)count * (op == FIT_XCHG_ALLGATHER_U64 ? c->world : 1);
    if (c->h_x.ensure(bytes)) return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->h_x.p, dbuf, bytes, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    if (c->xchg(c->xchg_user, op, c->h_x.p, count) != 0)
        return fail(FIT_E_RCCL, "host exchange op %d failed", op);
    HIP_TRY(hipMemcpyAsync(dbuf, c->h_x.p, bytes, hipMemcpyHostToDevice, c->st));
    return 0;
}

// ------------------------------------------------------------- persistent engine path
const char* trip_site_name(unsigned s) {
    switch (s) {
        case TRIP_WORKER_RING: return "scan worker waiting for a task";
        case TRIP_ROUND_START: return "committer waiting for the round before last";
        case TRIP_HELPER_TILE: return "commit helper waiting for a scan tile";
        case TRIP_HELPER_SNAP: return "commit helper waiting for the decider";
        case TRIP_DECIDER_REC: return "decider waiting for a helper record";
        case TRIP_SINGLE_TILE: return "single-wave commit waiting for a scan tile";
        case TRIP_NO_PROGRESS: return "round resolved no job";
        case TRIP_NO_KERNEL: return "no scan kernel for the key count";
        default: return "unknown";
    }
}

// The launch's error word and first trip record (read back with it): FIT_E_HIP with every field.
int trip_error(fit_ctx* c, const char* engine) {
    const TripRec& t = *c->h_trip.p;
    return fail(FIT_E_HIP,
                "%s watchdog tripped (code %u): site %u (%s), component %u, round %u, arg %u, "
                "block %u, q_head %u, q_tail %u, pubt %u, tdone %u / need %u, waited %.3f ms, "
                "%.3f ms into the launch (deadline %.3f ms)",
                engine, c->h_err.p[0], t.site, trip_site_name(t.site), t.comp, t.round, t.arg,
                t.block, t.q_head, t.q_tail, t.pubt, t.tdone, t.need, t.waited / 1e5, t.when / 1e5,
                c->wd_ticks / 1e5);
}
// ---- what the two persistent engines (k_engine, k_engine_tl) share on the host ----------------
// The launch's components: those with jobs that this rank owns, launch component i = comps[i].
struct EngineComps {
    std::vector<int> comps;
    int nc = 0;
    int32_t maxnodes = 0;  // largest of them (nodes)
    int64_t wcap = 0;      // window cap: the engines' per-tile counters hold 128 job tiles
};

EngineComps engine_comps(fit_ctx* c, const std::vector<int32_t>& jb, const std::vector<char>& owned) {
    EngineComps E;
    for (int k = 0; k < c->ncomp; ++k)
        if (owned[k] && jb[k + 1] > jb[k]) {
            E.comps.push_back(k);
            E.maxnodes = std::max(E.maxnodes, c->nb[k + 1] - c->nb[k]);
        }
    E.nc = (int)E.comps.size();
    E.wcap = std::min(c->wmax, 8192);
    return E;
}

// One CompOut per launch component into the placement's stats; every component must have
// resolved all its jobs.
int fold_comp_out(fit_ctx* c, const std::vector<int32_t>& jb, const std::vector<int>& comps, fit_stats& S) {
    double commit_max = 0;
    for (size_t i = 0; i < comps.size(); ++i) {
        const CompOut& o = c->h_eco.p[i];
        const int k = comps[i];
        if (o.done_jobs != jb[k + 1] - jb[k])
            return fail(FIT_E_HIP, "component %d resolved %lld of %d jobs", k, (long long)o.done_jobs,
                        jb[k + 1] - jb[k]);
        S.placed += o.placed;
        S.rounds = std::max<int64_t>(S.rounds, o.rounds);
        S.stops_rescan += o.stops_rescan;
        S.stops_dirty += o.stops_dirty;
        commit_max = std::max(commit_max, o.t_commit / 1e5);
    }
    S.ms_commit += commit_max;
    return 0;
}

// The launch's buffers, its CompState rows and the task-ring check.  `keys`: candidate entries per
// job (block-slices x keys per slice); slice(len, s) sets s.ks, s.sub and s.nslice for a component
// of len nodes.
template <class Slice>
int engine_plan(fit_ctx* c, const std::vector<int32_t>& jb, const EngineComps& E, int64_t keys, Slice slice) {
    const int nc = E.nc;
    const int64_t wcap = E.wcap, per_comp_cand = wcap * keys;
    // two sets of per-round buffers (plans, candidates, bounds, job rows) by round parity
    // (fit_engine_ctl.h): a round starts while the previous round's last tiles are still scanned
    if (c->ecs.ensure(nc) || c->eco.ensure(nc) || c->h_ecs.ensure(nc) || c->h_eco.ensure(nc) ||
        c->plan.ensure(2 * nc) ||
        c->cand.ensure((size_t)2 * nc * per_comp_cand + (size_t)2 * nc * PAIR_AREA) ||
        c->bnd.ensure((size_t)2 * nc * wcap) || c->wjob.ensure((size_t)2 * nc * wcap) ||
        c->ectl.ensure(engine_ctl_bytes()) || c->ering.ensure(engine_ring_bytes()) ||
        c->h_err.ensure(4))
        return FIT_E_OOM;
    if ((int64_t)2 * nc * per_comp_cand + (int64_t)2 * nc * PAIR_AREA > INT32_MAX)
        return fail(FIT_E_INVAL, "candidate buffer exceeds 2^31 entries (%d components)", nc);
    int32_t max_slices = 1;
    for (int i = 0; i < nc; ++i) {
        const int k = E.comps[i];
        CompState& s = c->h_ecs.p[i];
        s.nb = s.sb = c->nb[k];
        s.ne = s.se = c->nb[k + 1];
        slice(s.ne - s.nb, s);
        s.onepart = c->comp_onepart[k] ? 1 : 0;
        max_slices = std::max(max_slices, s.nslice);
        s.jstart = jb[k];
        s.jend = jb[k + 1];
        s.cand_off = (int64_t)i * per_comp_cand;
        s.slot0 = (int32_t)(i * wcap);
        s.cand_alt = (int64_t)(nc + i) * per_comp_cand;
        s.slot_alt = (int32_t)((nc + i) * wcap);
        s.pair_off = (int32_t)(2 * nc * per_comp_cand + (int64_t)2 * i * PAIR_AREA);
        s.wmin = std::min(c->wmin, (int)wcap);
        s.wmax = (int32_t)wcap;
    }
    // task ring: a committer publishes a round only after all tiles of the round before last are
    // done, so at most 2 * nc * job tiles * slices tiles are outstanding; the ring must hold them
    // all (a granule overwritten before its worker read it would be lost)
    // (+ one tile: a round's first tile may be scanned as twice the slices, K_T0PAIR / TL_T0PAIR)
    if ((int64_t)2 * ring_comps(nc) * ((wcap + SCAN_JOBS - 1) / SCAN_JOBS + 1) * max_slices >
        (int64_t)engine_ring_tasks())
        return fail(FIT_E_INVAL, "task ring too small: %d components x %lld tiles x %d slices",
                    nc, (long long)((wcap + SCAN_JOBS - 1) / SCAN_JOBS), max_slices);
    return 0;
}

// The launch itself: CompState upload and the control-block, ring and bound resets, then, under
// the device lock (one persistent launch per device at a time, see DevArb) from before the launch
// to the synchronisation that ends it, launch() between two events and the read-back of CompOut,
// the workers' counters, the error word and the first trip record.  settle(trip_rc) recovers: it
// gets the trip's error code (0: no trip) and returns the call's.  Then the stats.
template <class Launch, class Settle>
int engine_launch(fit_ctx* c, const std::vector<int32_t>& jb, const EngineComps& E, int workers,
                  const char* name, Launch launch, Settle settle, fit_stats& S) {
    const int nc = E.nc;
    hipStream_t st = c->st;
    if (c->ebusy.ensure(2 * workers) || c->h_ebusy.ensure(2 * workers) || c->h_trip.ensure(1))
        return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->ecs.p, c->h_ecs.p, sizeof(CompState) * nc, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(c->ectl.p, 0, engine_ctl_bytes(), st));
    HIP_TRY(hipMemsetAsync(c->ering.p, 0, engine_ring_bytes(), st));
    // every bound KEY_INF: a round resets only the bounds its buffer set's last round used
    HIP_TRY(hipMemsetAsync(c->bnd.p, 0xff, sizeof(uint64_t) * 2 * nc * E.wcap, st));
    {
        ArbGuard arb;
        int rc = arb.take(c->device);
        if (rc) return rc;
        S.ms_arb_wait = arb.waited_ms;
        HIP_TRY(hipEventRecord(c->ev[0], st));
        rc = launch();
        if (rc) return rc;
        HIP_TRY(hipEventRecord(c->ev[1], st));
        HIP_TRY(hipMemcpyAsync(c->h_eco.p, c->eco.p, sizeof(CompOut) * nc, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(c->h_ebusy.p, c->ebusy.p, sizeof(int64_t) * 2 * workers,
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(c->h_err.p, c->ectl.p + engine_ctl_error_offset(), 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(c->h_trip.p, c->ectl.p + engine_ctl_trip_offset(), sizeof(TripRec),
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    }
    if (int rc = settle(c->h_err.p[0] ? trip_error(c, name) : 0)) return rc;
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    S.ms_device += ms;
    int64_t busy = 0;
    // per worker {busy ticks, evaluations scanned}: tiles of a finished round are dropped, so
    // the performed evaluations are counted where they happen
    for (int i = 0; i < workers; ++i) {
        busy += c->h_ebusy.p[2 * i];
        S.evals += c->h_ebusy.p[2 * i + 1];
    }
    S.ms_scan += busy / 1e5 / workers;  // average worker busy time (100 MHz ticks)
    return fold_comp_out(c, jb, E.comps, S);
}

// All rounds of all owned components in one launch (fit_persistent.hip).
int run_persistent(fit_ctx* c, const std::vector<int32_t>& jb, const std::vector<char>& owned,
                   const int32_t* cpu, const int32_t* mem, const int32_t* gpu, const int32_t* wall,
                   const uint16_t* part, const uint16_t* nk, int32_t* out, int32_t kmax,
                   fit_stats& S) {
    hipStream_t st = c->st;
    const EngineComps E = engine_comps(c, jb, owned);
    const int nc = E.nc;
    if (nc == 0) return 0;
    // keys per block-slice: KS, halved (slices doubled, the same MAX_SLICES * KS candidates per
    // job) while a wave's sub-slice would exceed sub_target nodes — a round's first job tile, which
    // the commit waits for, then spreads over more blocks.  C3o (one 100k-node component): KS 16
    // 552 ms, 8 471 ms, 4 441 ms, 2 480 ms (the bound B, a minimum over more slices of fewer keys,
    // turns tight: 891 rescans); C3 / C2 components stay at KS (sub-slices of 98 / 64 nodes).
    int sub_target = 256, ks_min = 4;
    if (const char* e = getenv("FIT_SUB_TARGET")) sub_target = std::max(MIN_SUB, atoi(e));
    if (const char* e = getenv("FIT_KS_MIN")) ks_min = std::max(2, std::min(KS, atoi(e)));
    // a multi-node job needs k keys <= B on one slice: the slice that sets B has ks of them, all
    // clean when the job opens a round, so ks >= kmax keeps every round's first job resolvable
    while (ks_min < kmax) ks_min *= 2;
    int rc = engine_plan(c, jb, E, (int64_t)MAX_SLICES * KS, [&](int32_t len, CompState& s) {
        for (s.ks = KS;; s.ks /= 2) {
            const int slices = MAX_SLICES * KS / s.ks;
            s.sub = std::max(MIN_SUB, (len + SCAN_WAVES * slices - 1) / (SCAN_WAVES * slices));
            s.nslice = std::max(1, (len + SCAN_WAVES * s.sub - 1) / (SCAN_WAVES * s.sub));
            if (s.sub <= sub_target || s.ks / 2 < ks_min) break;
        }
    });
    if (rc) return rc;
    size_t lds = engine_lds_bytes(E.maxnodes);
    // experiment knob: a larger LDS request caps the blocks per CU (e.g. > 80 KB: one per CU)
    if (const char* e = getenv("FIT_ENGINE_LDS_MIN")) lds = std::max(lds, (size_t)atol(e));
    int per_cu = engine_blocks_per_cu(lds);
    if (per_cu <= 0) return fail(FIT_E_HIP, "k_engine does not fit on a CU (lds %zu)", lds);
    // Only the committers (blocks [0, nc), dispatched first) must be co-resident: a worker block
    // that is not yet resident has claimed no task, so nobody waits on it.  One block per CU:
    // the scan workers are mostly idle already, and a second block on a committer's CU slows
    // the serial commit chain (measured: 2/CU → commit +3%, no scan gain).
    int workers = std::max(8, std::max(1, per_cu - 1) * c->cus - nc);
    if (const char* e = getenv("FIT_WORKERS")) workers = std::max(1, atoi(e));
    // the node rows as they were: a trip leaves them partly committed, and the context must stay
    // usable after FIT_E_HIP (restored below)
    EngineCompIds ids;  // launch component -> component id (the rows of jmin)
    memset(&ids, 0, sizeof ids);
    for (int i = 0; i < nc; ++i) ids.id[i] = (int8_t)E.comps[i];
    static const bool no_backup = getenv("FIT_REC_BACKUP") && atoi(getenv("FIT_REC_BACKUP")) == 0;  // A/B only
    if (c->rec_bak.ensure(std::max(c->nn, 1))) return FIT_E_OOM;
    if (!no_backup)
        HIP_TRY(hipMemcpyAsync(c->rec_bak.p, c->rec.p, sizeof(NodeRec) * c->nn, hipMemcpyDeviceToDevice, st));
    return engine_launch(
        c, jb, E, workers, "placement engine",
        [&]() -> int {
            HIP_TRY(launch_engine(nc + workers, lds, st, c->ectl.p, c->ering.p, c->ecs.p, c->eco.p,
                                  c->plan.p, nc, c->rec.p, c->jl.p, cpu, mem, gpu, wall, part, nk,
                                  c->cand.p, c->bnd.p, c->wjob.p, out, kmax, c->ebusy.p, c->jpk.p,
                                  c->wd_ticks, c->jmin.p, ids));
            return 0;
        },
        [&](int trip) -> int {
            if (!trip) return 0;
            if (no_backup) {  // no copy was taken: the rows are partly committed, drop the table
                c->have_nodes = c->have_tl = false;
                return trip;
            }
            HIP_TRY(hipMemcpyAsync(c->rec.p, c->rec_bak.p, sizeof(NodeRec) * c->nn, hipMemcpyDeviceToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
            return trip;
        },
        S);
}

// The demand-class engine (fit_class.hip): one workgroup per component, no
// cross-block waits (so no launch arbitration), then the positions it wrote become node ids.
int run_class(fit_ctx* c, int32_t J, const std::vector<int32_t>& jb, const std::vector<char>& owned,
              const int32_t* wall, const uint16_t* nk, int32_t* out, int32_t kmax, fit_stats& S) {
    const int C = c->ncomp;
    hipStream_t st = c->st;
    if (c->eco.ensure(C) || c->h_eco.ensure(C) || c->cls_err.ensure(1) || c->h_cls_err.ensure(1) ||
        c->rec_bak.ensure(std::max(c->nn, 1)))
        return FIT_E_OOM;
    int32_t* jbd = c->jls.p + joblists_scratch_ints(J) + 2;
    HIP_TRY(hipMemsetAsync(c->cls_err.p, 0, sizeof(unsigned), st));
    HIP_TRY(hipMemcpyAsync(c->rec_bak.p, c->rec.p, sizeof(NodeRec) * c->nn, hipMemcpyDeviceToDevice, st));
    const size_t lds = class_lds_bytes(c->cls_maxn);
    HIP_TRY(hipEventRecord(c->ev[0], st));
    uint32_t own = 0;  // components this rank places (component sharding; all at world 1)
    for (int k = 0; k < C; ++k)
        if (owned[k]) own |= 1u << k;
    HIP_TRY(launch_class(st, C, lds, c->rec.p, c->nb.data(), own, jbd, c->jl.p, wall, nk, c->jcls.p,
                         c->cls_dem.p, c->cls_n.p, kmax, out, c->eco.p, c->cls_err.p));
    HIP_TRY(hipEventRecord(c->ev[1], st));
    HIP_TRY(launch_class_out(st, out, (int64_t)J * kmax, c->rec.p));
    HIP_TRY(hipMemcpyAsync(c->h_eco.p, c->eco.p, sizeof(CompOut) * C, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(c->h_cls_err.p, c->cls_err.p, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (c->h_cls_err.p[0]) {
        HIP_TRY(hipMemcpyAsync(c->rec.p, c->rec_bak.p, sizeof(NodeRec) * c->nn, hipMemcpyDeviceToDevice, st));
        HIP_TRY(hipStreamSynchronize(st));
        return fail(FIT_E_HIP, "class engine: an in-block wait exceeded its bound (error %u)", c->h_cls_err.p[0]);
    }
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    S.ms_device += ms;
    double commit_max = 0;
    for (int k = 0; k < C; ++k) {
        if (!owned[k]) continue;
        const CompOut& o = c->h_eco.p[k];
        if (o.done_jobs != jb[k + 1] - jb[k])
            return fail(FIT_E_HIP, "component %d resolved %lld of %d jobs", k, (long long)o.done_jobs,
                        jb[k + 1] - jb[k]);
        S.placed += o.placed;
        S.evals += o.evals;
        S.rounds = std::max<int64_t>(S.rounds, o.rounds);   // set refills (longest component)
        S.stops_rescan += o.stops_rescan;                   // exact-scan resolutions
        S.stops_dirty += o.stops_dirty;
        commit_max = std::max(commit_max, o.t_commit / 1e5);
    }
    S.ms_commit += commit_max;
    S.engine = 3;
    return 0;
}

// The demand classes of every component's jobs (k_classify, fit_class.hip), enqueued; the class
// counts are in h_cls_n after the next synchronisation, for classes_fit.
int enqueue_classify(fit_ctx* c, int32_t J, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                     const uint16_t* part) {
    const int C = c->ncomp;
    hipStream_t st = c->st;
    const size_t ts = (size_t)C * class_table_slots() * class_slot_bytes();
    if (c->jcls.ensure(std::max(J, 1)) || c->cls_tab.ensure(ts) || c->cls_dem.ensure((size_t)C * class_max()) ||
        c->cls_n.ensure(C) || c->h_cls_n.ensure(C))
        return FIT_E_OOM;
    HIP_TRY(hipMemsetAsync(c->cls_tab.p, 0, ts, st));
    HIP_TRY(hipMemsetAsync(c->cls_n.p, 0, sizeof(int32_t) * C, st));
    HIP_TRY(launch_classify(st, c->jcomp.p, cpu, mem, gpu, part, J, c->cls_tab.p, c->cls_dem.p, c->cls_n.p,
                            c->jcls.p));
    HIP_TRY(hipMemcpyAsync(c->h_cls_n.p, c->cls_n.p, sizeof(int32_t) * C, hipMemcpyDeviceToHost, st));
    return 0;
}

// whether every component has at most class_max() demand classes
bool classes_fit(const fit_ctx* c) {
    for (int k = 0; k < c->ncomp; ++k)
        if (c->h_cls_n.p[k] > class_max()) return false;
    return true;
}

// Per-component job lists in priority order (stable), built on the device from the prefilter's
// component ids (launch_joblists: counting sort by component); only the component offsets and
// two counters come back to the host.  jb[k] .. jb[k+1] = component k's list range.
// With `classify` the demand classes of every component's jobs are counted in the same
// synchronisation (k_classify, fit_class.hip); *cls_ok says whether every component has at most
// class_max() of them.
int build_job_lists(fit_ctx* c, int32_t J, fit_stats& S, std::vector<int32_t>& jb,
                    const int32_t* cpu = nullptr, const int32_t* mem = nullptr, const int32_t* gpu = nullptr,
                    const uint16_t* part = nullptr, bool classify = false, bool* cls_ok = nullptr) {
    const int C = c->ncomp;
    hipStream_t st = c->st;
    if (c->jl.ensure(std::max(J, 1)) || c->jpk.ensure(J + 1) ||
        c->jls.ensure(std::max<size_t>(joblists_scratch_ints(J), 1) + 2 * (C + 1) + 2) ||
        c->h_jls.ensure(2 * (C + 1) + 2))
        return FIT_E_OOM;
    int32_t* g = c->jls.p + joblists_scratch_ints(J);
    int32_t* jbd = g + 2;
    int32_t* mbd = jbd + C + 1;
    HIP_TRY(launch_joblists(st, c->jcomp.p, J, C, c->jls.p, g, jbd, mbd, c->jl.p, c->jpk.p));
    // the counters, the component offsets and the multi-node offsets (mbd[C]: multi-node jobs)
    HIP_TRY(hipMemcpyAsync(c->h_jls.p, g, sizeof(int32_t) * (2 * (C + 1) + 2), hipMemcpyDeviceToHost, st));
    if (classify) {
        const int rc = enqueue_classify(c, J, cpu, mem, gpu, part);
        if (rc) return rc;
    }
    HIP_TRY(hipStreamSynchronize(st));
    if (c->h_jls.p[1]) return fail(FIT_E_INVAL, "a job has a negative demand or nodes_k > kmax");
    if (cls_ok) *cls_ok = classify && classes_fit(c);
    S.rejected = c->h_jls.p[0];
    jb.assign(c->h_jls.p + 2, c->h_jls.p + 2 + C + 1);
    c->last_multi = c->h_jls.p[2 + C + 1 + C];
    for (int k = 0; k < C; ++k) S.useful_evals += (int64_t)(jb[k + 1] - jb[k]) * c->n;
    return 0;
}

// The demand classes of every component's jobs on their own (after build_job_lists, which counted
// the multi-node jobs the automatic choice needs): k_classify and one synchronisation.
int classify_jobs(fit_ctx* c, int32_t J, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                  const uint16_t* part, bool* cls_ok) {
    const int rc = enqueue_classify(c, J, cpu, mem, gpu, part);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));
    *cls_ok = classes_fit(c);
    return 0;
}

// ------------------------------------------------------------------------ placement
// A small placement in one launch (k_small, fit_kernels.hip: prefilter, per-component job order
// and placement in one kernel) and ONE device-to-host copy: with host memory for the placements
// (h_out) the stats ride at the tail of the out buffer (fit_place sizes it), so placements and
// stats come back together into pinned memory.
// Wait for the stream's work up to now: a short spin on an event (a small placement takes tens of
// µs, the wake-up of a blocking synchronisation costs about as much), then the blocking wait.
hipError_t sync_small(fit_ctx* c) {
    if (c->sync_spin) {
        hipError_t e = hipEventRecord(c->ev[2], c->st);
        if (e != hipSuccess) return e;
        const double t0 = now_ms();
        while ((e = hipEventQuery(c->ev[2])) == hipErrorNotReady && now_ms() - t0 < 2.0) {
        }
        if (e != hipErrorNotReady) return e;
    }
    return hipStreamSynchronize(c->st);
}

int place_direct(fit_ctx* c, int32_t J, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                 const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax,
                 int32_t* out, int32_t* h_out, fit_stats& S, const SmallBatch* hb = nullptr) {
    const int C = c->ncomp;
    const int G = std::max(C, 1);  // blocks (block 0 also when the table is empty)
    hipStream_t st = c->st;
    const size_t rows = (size_t)J * kmax;
    const size_t nback = (h_out ? rows : 0) + 2 + G;
    if (c->small_placed.ensure(2 + G) || c->h_small.ensure(nback)) return FIT_E_OOM;
    int32_t* stat = h_out ? out + rows : c->small_placed.p;
    SmallComps sc;
    for (int k = 0; k <= 32; ++k) sc.nb[k] = c->nb[std::min(k, C)];
    HIP_TRY(hipEventRecord(c->ev[0], st));
    if (hb)
        HIP_TRY(launch_small_args(st, C, c->rec.p, sc, c->d_ptab.p, c->np, *hb, nk != nullptr, J, kmax, out, stat));
    else
        HIP_TRY(launch_small(st, C, c->rec.p, sc, c->d_ptab.p, c->np, cpu, mem, gpu, wall, part, nk, J, kmax,
                             out, stat));
    HIP_TRY(hipEventRecord(c->ev[1], st));
    HIP_TRY(hipMemcpyAsync(c->h_small.p, h_out ? out : stat, sizeof(int32_t) * nback, hipMemcpyDeviceToHost,
                           st));
    HIP_TRY(sync_small(c));
    const int32_t* hs = c->h_small.p + (h_out ? rows : 0);
    if (hs[1]) return fail(FIT_E_INVAL, "a job has a negative demand or nodes_k > kmax");
    if (h_out) memcpy(h_out, c->h_small.p, sizeof(int32_t) * rows);
    S.rejected = hs[0];
    for (int k = 0; k < C; ++k) S.placed += hs[2 + k];
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    S.ms_device = S.ms_commit = ms;
    S.rounds = C > 0 && J > S.rejected ? 1 : 0;
    S.components = C;
    S.engine = 2;
    return 0;
}

// The host-driven speculative rounds, shared by the plain fit and the backfill:
// per round the plans of every component's window, scan(blocks, this rank's candidate section),
// the exchange when the nodes are sharded over ranks, commit(entries per lane, largest component
// with a window, candidates per rank, ranks) and the windows' update from the results.  `keys`
// per (job, block-slice), at most `slices` block-slices per job per rank of >= min_sub nodes per
// wave; only `owned` components get a window.
template <class Scan, class Commit>
int run_rounds(fit_ctx* c, const std::vector<int32_t>& jb, const std::vector<char>& owned, bool node_sharded,
               int keys, int slices, int min_sub, Scan scan, Commit commit, fit_stats& S) {
    const int C = c->ncomp;
    hipStream_t st = c->st;
    const int shards = node_sharded ? c->world : 1;
    const int srank = node_sharded ? c->rank : 0;
    std::vector<int32_t> cur(jb.begin(), jb.end() - 1), win(C, c->wmin);
    if (c->plan.ensure(C + 1) || c->res.ensure(C + 1) || c->h_plan.ensure(C + 1) ||
        c->h_res.ensure(C + 1))
        return FIT_E_OOM;
    float ms;
    for (;;) {
        int64_t blocks = 0, slots = 0, cand_n = 0, evals = 0;
        int epl = 1;
        int32_t maxlen = 0;
        for (int k = 0; k < C; ++k) {
            CompPlan& P = c->h_plan.p[k];
            memset(&P, 0, sizeof P);
            P.nb = c->nb[k];
            P.ne = c->nb[k + 1];
            const int32_t len = P.ne - P.nb;
            const int32_t per = (len + shards - 1) / shards;
            P.sb = std::min(P.ne, P.nb + per * srank);
            P.se = std::min(P.ne, P.sb + per);
            P.ks = keys;
            P.sub = std::max(min_sub, (per + SCAN_WAVES * slices - 1) / (SCAN_WAVES * slices));
            P.nslice = std::max(1, (per + SCAN_WAVES * P.sub - 1) / (SCAN_WAVES * P.sub));
            epl = std::max(epl, (shards * P.nslice * keys + 63) / 64);
            P.jbase = cur[k];
            P.w = owned[k] ? std::min(win[k], jb[k + 1] - cur[k]) : 0;
            P.blk0 = (int32_t)blocks;
            P.cand_off = cand_n;
            P.slot0 = (int32_t)slots;
            if (P.w > 0) {
                blocks += (int64_t)((P.w + SCAN_JOBS - 1) / SCAN_JOBS) * P.nslice;
                cand_n += (int64_t)P.w * P.nslice * keys;
                slots += P.w;
                evals += (int64_t)P.w * (P.se - P.sb);
                maxlen = std::max(maxlen, len);
            }
        }
        if (slots == 0) break;
        S.rounds++;
        S.evals += evals;
        if (c->cand.ensure((size_t)cand_n * shards) || c->bnd.ensure(slots) ||
            c->wjob.ensure(slots))
            return FIT_E_OOM;
        HIP_TRY(hipMemcpyAsync(c->plan.p, c->h_plan.p, sizeof(CompPlan) * C, hipMemcpyHostToDevice,
                               st));
        HIP_TRY(hipMemsetAsync(c->bnd.p, 0xff, sizeof(uint64_t) * slots, st));
        HIP_TRY(hipEventRecord(c->ev[0], st));
        HIP_TRY(scan((int)blocks, c->cand.p + (size_t)srank * cand_n));
        HIP_TRY(hipEventRecord(c->ev[1], st));
        if (node_sharded) {
            // every rank scanned its node shard: gather all candidate sections, min the bounds
            int rc = xchg(c, FIT_XCHG_ALLGATHER_U64, c->cand.p, cand_n);
            if (!rc) rc = xchg(c, FIT_XCHG_MIN_U64, c->bnd.p, slots);
            if (rc) return rc;
        }
        HIP_TRY(hipEventRecord(c->ev[2], st));
        HIP_TRY(commit(epl, maxlen, cand_n, shards));
        HIP_TRY(hipEventRecord(c->ev[3], st));
        HIP_TRY(hipMemcpyAsync(c->h_res.p, c->res.p, sizeof(CommitResult) * C,
                               hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        S.ms_scan += ms;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[1], c->ev[2]));
        S.ms_exchange += ms;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
        S.ms_commit += ms;
        for (int k = 0; k < C; ++k) {
            const CompPlan& P = c->h_plan.p[k];
            if (P.w == 0) continue;
            const CommitResult& R = c->h_res.p[k];
            if (R.done < 0 || R.done > P.w)
                return fail(FIT_E_HIP, "commit returned %d of window %d", R.done, P.w);
            cur[k] += R.done;
            S.placed += R.placed;
            if (R.stop == 1) S.stops_rescan++;
            if (R.stop == 2) S.stops_dirty++;
            const int32_t nw = R.stop ? 2 * R.done : 2 * P.w;
            win[k] = std::max(c->wmin, std::min(c->wmax, nw));
        }
    }
    S.ms_device = S.ms_scan + S.ms_exchange + S.ms_commit;
    return 0;
}

int place_impl(fit_ctx* c, int32_t J, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
               const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax,
               int32_t* out, fit_stats* stats, int32_t* h_out = nullptr, bool* h_out_done = nullptr,
               const SmallBatch* hb = nullptr) {
    const double t0 = now_ms();
    fit_stats S;
    memset(&S, 0, sizeof S);
    S.jobs = J;
    hipStream_t st = c->st;
    if (J <= c->small_direct && !c->collective()) {  // a few jobs: one launch, one synchronisation
        const int rc = place_direct(c, J, cpu, mem, gpu, wall, part, nk, kmax, out, h_out, S, hb);
        if (rc) return rc;
        if (h_out_done) *h_out_done = h_out != nullptr;
        S.unplaced = J - S.placed - S.rejected;
        S.ms_total = now_ms() - t0;
        if (stats) *stats = S;
        return 0;
    }
    // 1. prefilter: out[] init, FIT_REJECTED, component per job
    // (and each component's minimum demands, for the persistent engine's recycling)
    if (c->jcomp.ensure(std::max(J, 1)) || c->jmin.ensure(3 * ENGINE_MAXC)) return FIT_E_OOM;
    HIP_TRY(hipMemsetAsync(c->jmin.p, JMIN_FILL, sizeof(int32_t) * 3 * ENGINE_MAXC, st));
    HIP_TRY(launch_prefilter(st, cpu, mem, gpu, wall, part, nk, J, kmax, c->d_ptab.p, c->np, out,
                             c->jcomp.p, c->jmin.p));
    // 2. per-component job lists in priority order (stable)
    const int C = c->ncomp;
    std::vector<int32_t> jb;
    // the demand-class engine needs the class count of every component: counted in the job
    // lists' synchronisation when the node table qualifies (world > 1: component sharding only —
    // the node-sharded layout keeps the host-driven rounds)
    const int pre_mode = !c->collective() ? 0
                         : (c->shard_mode == FIT_SHARD_AUTO ? (C >= c->world ? FIT_SHARD_COMPONENTS : FIT_SHARD_NODES)
                                                            : c->shard_mode);
    const bool cls_able = c->cls_nodes_ok && pre_mode != FIT_SHARD_NODES;
    const bool try_cls = (c->cls_mode == 1 || c->cls_mode == 2) && cls_able && (c->cls_mode == 2 || J > c->small_batch);
    bool cls_ok = false;
    int rc0 = build_job_lists(c, J, S, jb, cpu, mem, gpu, part, try_cls, &cls_ok);
    if (rc0) return rc0;
    // automatic (cls_mode 3, the default): a large placement whose live jobs are mostly multi-node
    // (C4) runs the class engine — its all-picks-at-once commit beats the persistent engine's
    // single-wave commit there; k = 1 queues keep the persistent engine
    const int32_t live = J - S.rejected;
    if (c->cls_mode == 3 && cls_able && live > c->small_batch && 2 * (int64_t)c->last_multi >= live) {
        rc0 = classify_jobs(c, J, cpu, mem, gpu, part, &cls_ok);
        if (rc0) return rc0;
    }
    const bool use_cls = cls_ok && (c->cls_mode == 2 || live > c->small_batch);

    // world > 1: split by components (each rank owns whole components, no per-round exchange)
    // or by nodes (north_star: every rank scans 1/world of every component, RCCL each round)
    int mode = 0;
    std::vector<char> owned(C, 1);
    if (c->collective()) {
        mode = c->shard_mode;
        if (mode == FIT_SHARD_AUTO) mode = C >= c->world ? FIT_SHARD_COMPONENTS : FIT_SHARD_NODES;
        if (mode == FIT_SHARD_COMPONENTS) {
            // LPT by work (jobs × nodes); identical on every rank (same inputs, same order)
            std::vector<int> order(C);
            for (int k = 0; k < C; ++k) order[k] = k;
            auto work = [&](int k) { return (int64_t)(jb[k + 1] - jb[k]) * (c->nb[k + 1] - c->nb[k]); };
            std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return work(a) > work(b); });
            std::vector<int64_t> load(c->world, 0);
            for (int k : order) {
                int r = (int)(std::min_element(load.begin(), load.end()) - load.begin());
                load[r] += work(k) + 1;
                owned[k] = r == c->rank;
            }
        }
    }
    S.shard_mode = mode;
    S.components = C;
    const bool node_sharded = mode == FIT_SHARD_NODES;

    // 3. speculative rounds: one persistent launch, or the host-driven loop (node sharding
    // exchanges candidates over RCCL every round, so it keeps the host loop; a small batch is
    // cheaper as a round or two of k_scan / k_commit than as a whole-chip persistent grid)
    const bool small = J - S.rejected <= c->small_batch;
    if (use_cls) {
        int rc = run_class(c, J, jb, owned, wall, nk, out, kmax, S);
        if (rc) return rc;
    } else if (c->persistent && !node_sharded && !small) {
        int rc = run_persistent(c, jb, owned, cpu, mem, gpu, wall, part, nk, out, kmax, S);
        if (rc) return rc;
        S.engine = 1;
    } else {
        int rc = run_rounds(
            c, jb, owned, node_sharded, KS, MAX_SLICES, MIN_SUB,
            [&](int blocks, uint64_t* cand) {
                return launch_scan(blocks, st, c->rec.p, c->jl.p, cpu, mem, gpu, wall, part, nk, c->plan.p, C,
                                   cand, c->bnd.p, c->wjob.p);
            },
            // the commit's dirty bitmap in LDS covers the largest component that has a window
            [&](int epl, int32_t maxlen, int64_t cand_n, int shards) {
                return launch_commit(C, epl, (size_t)((maxlen + 31) / 32) * 4, st, c->rec.p, c->plan.p,
                                     c->cand.p, cand_n, shards, c->bnd.p, c->wjob.p, out, kmax, c->res.p);
            },
            S);
        if (rc) return rc;
    }  // host-driven rounds
    if (mode == FIT_SHARD_COMPONENTS) {
        // each rank placed only its components: combine placements (owner's >= -1 beats -1;
        // rejections are identical everywhere) and node rows (only owners lowered them)
        int rc = xchg(c, FIT_XCHG_MAX_I32, out, (int64_t)J * kmax);
        if (!rc) rc = xchg(c, FIT_XCHG_MIN_I32, c->rec.p, (int64_t)c->nn * 8);
        if (rc) return rc;
        // global placed count: allgather one u64 per rank, sum on the host
        if (c->xcount.ensure(c->world) || c->h_count.ensure(c->world)) return FIT_E_OOM;
        c->h_count.p[c->rank] = (uint64_t)S.placed;
        HIP_TRY(hipMemcpyAsync(c->xcount.p + c->rank, c->h_count.p + c->rank, 8,
                               hipMemcpyHostToDevice, st));
        rc = xchg(c, FIT_XCHG_ALLGATHER_U64, c->xcount.p, 1);
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(c->h_count.p, c->xcount.p, 8 * c->world, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        S.placed = 0;
        for (int r = 0; r < c->world; ++r) S.placed += (int64_t)c->h_count.p[r];
    }
    // jobs of partitions without nodes are FIT_UNPLACED like jobs nothing fits
    S.unplaced = J - S.placed - S.rejected;
    S.ms_total = now_ms() - t0;
    if (stats) *stats = S;
    return 0;
}

// ----------------------------------------------------------- time-windowed backfill
// SPEC §2b: the same speculative rounds as the plain fit (host-driven loop), with run-list
// scans / commits (fit_timeline.hip).  world > 1 always splits by nodes: every rank scans its
// share of each component, the candidate sections are exchanged each round and the identical
// deterministic commit runs on every rank over replicated run lists.
// Persistent single-launch backfill (k_engine_tl): the placement's rounds for
// every component in one launch, no host round trips (world == 1).
int run_persistent_tl(fit_ctx* c, const std::vector<int32_t>& jb, const int32_t* cpu,
                      const int32_t* mem, const int32_t* gpu, const int32_t* wall,
                      const uint16_t* part, int32_t* out, int32_t* outs, fit_stats& S) {
    hipStream_t st = c->st;
    const EngineComps E = engine_comps(c, jb, std::vector<char>(c->ncomp, 1));
    const int nc = E.nc;
    if (nc == 0) return 0;
    const int R = engine_tl_runs(E.maxnodes);
    if (R < 1) return fail(FIT_E_INVAL, "partition component of %d nodes is too large for the "
                                        "timeline engine's LDS", E.maxnodes);
    int slices = TL_SLICES, tl_min_sub = TL_MIN_SUB;
    if (const char* e = getenv("FIT_TL_SLICES")) slices = std::max(1, std::min(atoi(e), TL_SLICES));
    if (const char* e = getenv("FIT_TL_MINSUB")) tl_min_sub = std::max(1, atoi(e));
    int rc = engine_plan(c, jb, E, (int64_t)slices * TL_KS, [&](int32_t len, CompState& s) {
        s.ks = TL_KS;
        s.sub = std::max(tl_min_sub, (len + SCAN_WAVES * slices - 1) / (SCAN_WAVES * slices));
        s.nslice = std::max(1, (len + SCAN_WAVES * s.sub - 1) / (SCAN_WAVES * s.sub));
    });
    if (rc) return rc;
    const size_t lds = engine_tl_lds_bytes(E.maxnodes);
    // FIT_TL_SPLIT: committers and scan workers as two concurrent launches (fit_timeline.hip
    // k_engine_tl_t): the workers' launch carries only the scan's registers and LDS, so several
    // worker blocks share a CU instead of one block per CU for everything
    bool split = FIT_TL_SPLIT_DEF != 0;
    if (const char* e = getenv("FIT_TL_SPLIT")) split = atoi(e) != 0;
    const size_t lds_w = split ? engine_tl_scan_lds_bytes() : lds;
    const int per_cu = engine_tl_blocks_per_cu(lds, split ? 1 : 0);
    if (per_cu <= 0) return fail(FIT_E_HIP, "k_engine_tl does not fit on a CU (lds %zu)", lds);
    const int per_cu_w = split ? engine_tl_blocks_per_cu(lds_w, 2) : per_cu;
    if (per_cu_w <= 0) return fail(FIT_E_HIP, "k_engine_tl workers do not fit on a CU");
    int workers = split ? std::max(8, per_cu_w * std::max(1, c->cus - nc)) : std::max(8, per_cu * c->cus - nc);
    if (const char* e = getenv("FIT_WORKERS")) workers = std::max(1, atoi(e));
    if (split && !c->st2) {
        if (hipStreamCreateWithFlags(&c->st2, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming) != hipSuccess ||
            hipHostMalloc(&c->resident, 64, hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess)
            return fail(FIT_E_HIP, "split launch: stream / event / mapped flag");
    }
    // mode 0: committers and workers in one grid; 1: the committers; 2: the workers
    auto launch = [&](int blocks, size_t l, hipStream_t s, int mode, unsigned* dres) {
        return launch_engine_tl(blocks, l, s, c->ectl.p, c->ering.p, c->ecs.p, c->eco.p, c->plan.p, nc,
                                c->slab.p, c->tlhdr.p, c->jl.p, cpu, mem, gpu, wall, part, c->cand.p,
                                c->bnd.p, c->wjob.p, c->perm.p, out, outs, c->tl_slots, c->tl_slot_min, R,
                                c->ebusy.p, mode, dres, c->wd_ticks);
    };
    bool resident_late = false;
    rc = engine_launch(
        c, jb, E, workers, "timeline engine",
        [&]() -> int {
            if (!split) {
                HIP_TRY(launch(nc + workers, lds, st, 0, nullptr));
                return 0;
            }
            __atomic_store_n(c->resident, 0u, __ATOMIC_RELEASE);
            unsigned* dres = nullptr;
            HIP_TRY(hipHostGetDevicePointer(reinterpret_cast<void**>(&dres), c->resident, 0));
            HIP_TRY(launch(nc, lds, st, 1, dres));
            // the workers go in once every committer block holds its CU (a worker block on a CU
            // would leave a committer no room, and the committers' rounds wait for workers)
            const auto t0 = std::chrono::steady_clock::now();
            while (__atomic_load_n(c->resident, __ATOMIC_ACQUIRE) < (unsigned)nc) {
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(10)) {
                    resident_late = true;  // launched anyway: the kernels' own watchdogs end it
                    break;
                }
            }
            HIP_TRY(hipStreamWaitEvent(c->st2, c->ev[0], 0));  // after the control-block resets
            HIP_TRY(launch(workers, lds_w, c->st2, 2, nullptr));
            HIP_TRY(hipEventRecord(c->ev_join, c->st2));
            HIP_TRY(hipStreamWaitEvent(st, c->ev_join, 0));
            return 0;
        },
        // a trip leaves the run lists partly reserved: the timeline must be loaded again (a copy of
        // the slab per placement would cost more than the rare reload); the node table is untouched
        [&](int trip) -> int {
            if (trip || resident_late) c->have_tl = false;
            if (trip) return trip;
            if (resident_late) return fail(FIT_E_HIP, "timeline engine: committer blocks not resident after 10 s");
            return 0;
        },
        S);
    if (rc) return rc;
    S.engine = 1;
    return 0;
}

int place_tl_impl(fit_ctx* c, int32_t J, const int32_t* cpu, const int32_t* mem,
                  const int32_t* gpu, const int32_t* wall, const uint16_t* part, int32_t* out,
                  int32_t* outs, fit_stats* stats) {
    const double t0 = now_ms();
    fit_stats S;
    memset(&S, 0, sizeof S);
    S.jobs = J;
    hipStream_t st = c->st;
    if (c->jcomp.ensure(std::max(J, 1))) return FIT_E_OOM;
    HIP_TRY(launch_prefilter(st, cpu, mem, gpu, wall, part, nullptr, J, 1, c->d_ptab.p, c->np, out,
                             c->jcomp.p));
    if (J > 0) HIP_TRY(hipMemsetAsync(outs, 0xff, sizeof(int32_t) * J, st));
    const int C = c->ncomp;
    std::vector<int32_t> jb;
    int rc = build_job_lists(c, J, S, jb);
    if (rc) return rc;
    const bool node_sharded = c->collective();
    S.shard_mode = node_sharded ? FIT_SHARD_NODES : 0;
    S.components = C;
    if (c->persistent && !node_sharded && J - S.rejected > c->small_batch) {
        rc = run_persistent_tl(c, jb, cpu, mem, gpu, wall, part, out, outs, S);
        if (rc) return rc;
        S.unplaced = J - S.placed - S.rejected;
        S.ms_total = now_ms() - t0;
        if (stats) *stats = S;
        return 0;
    }
    int32_t maxlen = 1;
    for (int k = 0; k < C; ++k) maxlen = std::max(maxlen, c->nb[k + 1] - c->nb[k]);
    const size_t lds = commit_tl_lds_bytes(maxlen);
    const int runs = commit_tl_runs(maxlen);
    const int shards = node_sharded ? c->world : 1;
    // more, shorter block-slices than the plain fit: a run walk costs more per node, so the scan
    // wants more waves in flight; candidate entries per job stay <= 256
    int slices = std::max(1, TL_SLICES / shards), tl_min_sub = TL_MIN_SUB;
    if (const char* e = getenv("FIT_TL_SLICES")) slices = std::max(1, std::min(atoi(e), 512 / (TL_KS * shards)));
    if (const char* e = getenv("FIT_TL_MINSUB")) tl_min_sub = std::max(1, atoi(e));
    if (runs < 1)
        return fail(FIT_E_INVAL, "partition component of %d nodes is too large for the timeline "
                                 "commit's LDS", maxlen);
    rc = run_rounds(
        c, jb, std::vector<char>(C, 1), node_sharded, TL_KS, slices, tl_min_sub,
        [&](int blocks, uint64_t* cand) {
            return launch_scan_tl(blocks, st, c->slab.p, c->tlhdr.p, c->jl.p, cpu, mem, gpu, wall, part,
                                  c->plan.p, C, cand, c->bnd.p, c->wjob.p, c->tl_slots, c->tl_slot_min);
        },
        [&](int epl, int32_t, int64_t cand_n, int nshards) {
            return launch_commit_tl(C, epl, lds, st, c->slab.p, c->tlhdr.p, c->plan.p, c->cand.p, cand_n,
                                    nshards, c->bnd.p, c->wjob.p, c->perm.p, out, outs, c->res.p, c->tl_slots,
                                    runs);
        },
        S);
    if (rc) return rc;
    S.unplaced = J - S.placed - S.rejected;
    S.ms_total = now_ms() - t0;
    if (stats) *stats = S;
    return 0;
}

// ------------------------------------------------------------------------ fit_explain
// classify, (a long queue: the jobs in component order, launch_joblists),
// count, finalise — a fixed sequence of bounded launches on the context's stream, no host loop and
// no synchronisation in between; nothing here waits on another workgroup, so neither the watchdog
// nor the persistent-launch lock is involved.  Device pointers; *bad and the rows are valid once
// the caller has drained the stream.
static_assert(EX_FITS == FIT_WHY_FITS && EX_PARTITION == FIT_WHY_PARTITION && EX_LIMIT_TIME == FIT_WHY_LIMIT_TIME &&
                  EX_LIMIT_CPUS == FIT_WHY_LIMIT_CPUS && EX_LIMIT_MEM == FIT_WHY_LIMIT_MEM &&
                  EX_NO_NODES == FIT_WHY_NO_NODES && EX_RESOURCES == FIT_WHY_RESOURCES && FIT_KMAX == FIT_MAX_K,
              "fit_device.h and fitgpu.h disagree");
static_assert(sizeof(fit_why) == 32, "fit_why is 32 bytes");
// codes 1..4 of every family are LimitCode's by definition and pinned to fitgpu.h per family; 5 too:
static_assert(FIT_ETA_NO_NODES == FIT_WHY_NO_NODES && FIT_ROOM_NO_NODES == FIT_WHY_NO_NODES,
              "code 5 of FIT_ETA_* and FIT_ROOM_* is FIT_WHY_NO_NODES");
// below this many jobs the caller's order is kept: the sort's three launches cost more than the
// component passes a mixed wave adds
constexpr int32_t kExplainSortJobs = 256;

// A batch's job columns on the device (nk: nullptr without a nodes_k column).
struct JobCols {
    const int32_t *cpu, *mem, *gpu, *wall;
    const uint16_t *part, *nk;
};

// The query frame's host side.  The component node offsets as a kernel argument:
ExplainComps query_comps(const fit_ctx* c) {
    ExplainComps ec;
    ec.ncomp = c->ncomp;
    for (int k = 0; k <= 32; ++k) ec.nb[k] = c->nb[std::min(k, c->ncomp)];
    return ec;
}
// Above `threshold` jobs on several components, the classified jobs (c->jcomp) in component order
// (launch_joblists): *jl the list and *live its length on the device, the jobs that have a
// component; otherwise both nullptr, the caller's order.
int query_joblist(fit_ctx* c, int32_t J, int32_t threshold, const int32_t** jl, const int32_t** live) {
    const int C = c->ncomp;
    *jl = *live = nullptr;
    if (J <= threshold || C <= 1) return 0;
    if (c->jl.ensure(J) || c->jpk.ensure(J + 1) ||
        c->jls.ensure(std::max<size_t>(joblists_scratch_ints(J), 1) + 2 * (C + 1) + 2))
        return FIT_E_OOM;
    int32_t* g = c->jls.p + joblists_scratch_ints(J);
    int32_t* jbd = g + 2;
    HIP_TRY(launch_joblists(c->st, c->jcomp.p, J, C, c->jls.p, g, jbd, jbd + C + 1, c->jl.p, c->jpk.p));
    *jl = c->jl.p;
    *live = jbd + C;
    return 0;
}

// The sequence fit_explain, fit_when and fit_room share: the flag reset, classify() (rows' limit
// codes, component per job, *bad), above kExplainSortJobs jobs of several components the jobs in
// component order, then walk(components, job list, live count).
template <class Classify, class Walk>
int query_impl(fit_ctx* c, int32_t J, int32_t* bad, Classify classify, Walk walk) {
    if (c->jcomp.ensure(std::max(J, 1))) return FIT_E_OOM;
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), c->st));
    HIP_TRY(classify());
    const int32_t *jl, *live;
    if (const int rc = query_joblist(c, J, kExplainSortJobs, &jl, &live)) return rc;
    HIP_TRY(walk(query_comps(c), jl, live));
    return 0;
}

int explain_impl(fit_ctx* c, int32_t J, const JobCols& d, fit_why* out, int32_t* bad) {
    return query_impl(
        c, J, bad,
        [&] {
            return launch_explain_classify(c->st, c->d_ptab.p, c->np, d.cpu, d.mem, d.gpu, d.wall, d.part, d.nk, J,
                                           out, c->jcomp.p, bad);
        },
        [&](const ExplainComps& ec, const int32_t* jl, const int32_t* live) {
            return launch_explain(c->st, c->rec.p, ec, d.cpu, d.mem, d.gpu, d.wall, d.part, J, c->jcomp.p, jl, live,
                                  explain_slices(J, c->cls_maxn, c->cus), out);
        });
}

// --------------------------------------------------------------------------- fit_when
// fit_explain's sequence over the run lists instead of the node rows —
// classify, (a long queue: the jobs in component order), walk, finalise.  Bounded launches on the
// context's stream, nothing waits on another workgroup.  Device pointers; *bad and the rows are
// valid once the caller has drained the stream.
static_assert(ETA_NOW == FIT_ETA_NOW && ETA_PARTITION == FIT_ETA_PARTITION && ETA_LIMIT_TIME == FIT_ETA_LIMIT_TIME &&
                  ETA_LIMIT_CPUS == FIT_ETA_LIMIT_CPUS && ETA_LIMIT_MEM == FIT_ETA_LIMIT_MEM &&
                  ETA_NO_NODES == FIT_ETA_NO_NODES && ETA_LATER == FIT_ETA_LATER && ETA_HORIZON == FIT_ETA_HORIZON &&
                      ETA_WINDOW == FIT_ETA_WINDOW,
              "fit_device.h and fitgpu.h disagree");
static_assert(sizeof(fit_eta) == 32, "fit_eta is 32 bytes");
// nodes a wave walks at least before the node range is sliced further (explain_slices; fit_explain
// keeps 32 rows): a node costs a header load and a dependent load per four runs, so a short batch
// is latency-bound and wants the waves — 1,024 jobs on C5: 0.307 ms at 32, DESIGN.md §3.12 at 4
constexpr int kWhenMinNodes = 4;

int when_impl(fit_ctx* c, int32_t J, const JobCols& d, fit_eta* out, int32_t* bad) {
    return query_impl(
        c, J, bad,
        [&] {
            return launch_when_classify(c->st, c->d_ptab.p, c->np, d.cpu, d.mem, d.gpu, d.wall, d.part, J,
                                        c->tl_slot_min, out, c->jcomp.p, bad);
        },
        [&](const ExplainComps& ec, const int32_t* jl, const int32_t* live) {
            return launch_when(c->st, c->tlhdr.p, c->slab.p, ec, c->tl_slots, c->tl_slot_min, d.cpu, d.mem, d.gpu,
                               d.part, J, c->jcomp.p, jl, live,
                               explain_slices(J, c->cls_maxn, c->cus, kWhenMinNodes), out);
        });
}

// --------------------------------------------------------------------------- fit_room
// fit_explain's sequence with the room count in place of the shortage count
// — classify, (a long queue: the jobs in component order), count, finalise.  Bounded launches on
// the context's stream, nothing waits on another workgroup.  Device pointers; *bad and the rows are
// valid once the caller has drained the stream.
static_assert(ROOM_SOME == FIT_ROOM_SOME && ROOM_PARTITION == FIT_ROOM_PARTITION &&
                  ROOM_LIMIT_TIME == FIT_ROOM_LIMIT_TIME && ROOM_LIMIT_CPUS == FIT_ROOM_LIMIT_CPUS &&
                  ROOM_LIMIT_MEM == FIT_ROOM_LIMIT_MEM && ROOM_NO_NODES == FIT_ROOM_NO_NODES &&
                  ROOM_NONE == FIT_ROOM_NONE,
              "fit_device.h and fitgpu.h disagree");
static_assert(sizeof(struct fit_room) == 40 && offsetof(struct fit_room, copies) == 16 &&
                  offsetof(struct fit_room, best_node) == 24,
              "fit_room is 40 bytes, copies at 16");
static_assert(FIT_ROOM_UNBOUNDED == INT32_MAX, "FIT_ROOM_UNBOUNDED is INT32_MAX");

int room_impl(fit_ctx* c, int32_t J, const JobCols& d, struct fit_room* out, int32_t* bad) {
    return query_impl(
        c, J, bad,
        [&] {
            return launch_room_classify(c->st, c->d_ptab.p, c->np, d.cpu, d.mem, d.gpu, d.wall, d.part, J, out,
                                        c->jcomp.p, bad);
        },
        [&](const ExplainComps& ec, const int32_t* jl, const int32_t* live) {
            return launch_room(c->st, c->rec.p, ec, d.cpu, d.mem, d.gpu, d.wall, d.part, J, c->jcomp.p, jl, live,
                               explain_slices(J, c->cls_maxn, c->cus), out);
        });
}

// --------------------------------------------------------------------------- fit_preempt
// fit_room's sequence with the walk over each row's victims — classify, (a
// long queue: the jobs in component order), then per chunk of PRE_CHUNK positions walk and finalise.
// Bounded launches on the context's stream, nothing waits on another workgroup.  Device pointers;
// *bad and the rows are valid once the caller has drained the stream.
static_assert(PRE_FITS == FIT_PRE_FITS && PRE_PARTITION == FIT_PRE_PARTITION && PRE_LIMIT_TIME == FIT_PRE_LIMIT_TIME &&
                  PRE_LIMIT_CPUS == FIT_PRE_LIMIT_CPUS && PRE_LIMIT_MEM == FIT_PRE_LIMIT_MEM &&
                  PRE_NO_NODES == FIT_PRE_NO_NODES && PRE_EVICT == FIT_PRE_EVICT && PRE_NONE == FIT_PRE_NONE,
              "fit_device.h and fitgpu.h disagree");
static_assert(FIT_PRE_PARTITION == FIT_WHY_PARTITION && FIT_PRE_LIMIT_TIME == FIT_WHY_LIMIT_TIME &&
                  FIT_PRE_LIMIT_CPUS == FIT_WHY_LIMIT_CPUS && FIT_PRE_LIMIT_MEM == FIT_WHY_LIMIT_MEM &&
                  FIT_PRE_NO_NODES == FIT_WHY_NO_NODES,
              "codes 1..5 of FIT_PRE_* are FIT_WHY_*'s");
static_assert(sizeof(fit_evict) == 32 && offsetof(fit_evict, code) == 0 && offsetof(fit_evict, node) == 4 &&
                  offsetof(fit_evict, victims) == 8 && offsetof(fit_evict, top_prio) == 12 &&
                  offsetof(fit_evict, members) == 16 && offsetof(fit_evict, fit) == 20 &&
                  offsetof(fit_evict, able) == 24 && offsetof(fit_evict, outranked) == 28,
              "fit_evict is 32 bytes: code, node, victims, top_prio, then the four counters");

int preempt_impl(fit_ctx* c, int32_t J, const JobCols& d, const int32_t* prio, fit_evict* out, int32_t* bad) {
    const int S = preempt_slices(J, c->cls_maxn, c->cus);
    if (c->pe_part.ensure(preempt_partials(J, S))) return FIT_E_OOM;
    return query_impl(
        c, J, bad,
        [&] {
            return launch_preempt_classify(c->st, c->d_ptab.p, c->np, c->ncomp, d.cpu, d.mem, d.gpu, d.wall, d.part, J,
                                           out, c->jcomp.p, bad);
        },
        [&](const ExplainComps& ec, const int32_t* jl, const int32_t* live) {
            return launch_preempt(c->st, c->rec.p, c->voff.p, c->vent.p, ec, d.cpu, d.mem, d.gpu, d.wall, d.part, prio,
                                  J, c->jcomp.p, jl, live, S, c->pe_part.p, out);
        });
}

// --------------------------------------------------------------------------- fit_preempt_k
// fit_preempt's sequence, the walk keeping the kmax smallest keys per (job,
// node slice) instead of one.  Same bounded launches, slices and chunks.
static_assert(sizeof(fit_evict_k) == 40 && offsetof(fit_evict_k, code) == 0 && offsetof(fit_evict_k, need) == 4 &&
                  offsetof(fit_evict_k, evict_nodes) == 8 && offsetof(fit_evict_k, victims) == 12 &&
                  offsetof(fit_evict_k, top_prio) == 16 && offsetof(fit_evict_k, members) == 20 &&
                  offsetof(fit_evict_k, fit) == 24 && offsetof(fit_evict_k, able) == 28 &&
                  offsetof(fit_evict_k, outranked) == 32 && offsetof(fit_evict_k, reserved) == 36,
              "fit_evict_k is 40 bytes: code, need, evict_nodes, victims, top_prio, the four counters, reserved");

int preempt_k_impl(fit_ctx* c, int32_t J, const JobCols& d, const int32_t* prio, int32_t kmax, fit_evict_k* out,
                   int32_t* out_node, int32_t* out_vic, int32_t* bad) {
    const int S = preempt_slices(J, c->cls_maxn, c->cus);
    if (c->pe_part.ensure(preempt_k_partials(J, S, kmax))) return FIT_E_OOM;
    return query_impl(
        c, J, bad,
        [&] {
            return launch_preempt_k_classify(c->st, c->d_ptab.p, c->np, c->ncomp, d.cpu, d.mem, d.gpu, d.wall, d.part,
                                             d.nk, kmax, J, out, out_node, out_vic, c->jcomp.p, bad);
        },
        [&](const ExplainComps& ec, const int32_t* jl, const int32_t* live) {
            return launch_preempt_k(c->st, c->rec.p, c->voff.p, c->vent.p, ec, d.cpu, d.mem, d.gpu, d.wall, d.part,
                                    prio, kmax, J, c->jcomp.p, jl, live, S, c->pe_part.p, out, out_node, out_vic);
        });
}

// fit_load_victims / fit_load_victims_device behind their checks: the row-ordered offsets from the
// caller's (h_off: host copy, nullptr = every list empty), then the entries from the device CSR.
// The victims loaded before are replaced from the first write on.
int load_victims_impl(fit_ctx* c, const int32_t* h_off, const int32_t* off, const int32_t* prio, const int32_t* cpu,
                      const int32_t* mem, const int32_t* gpu) {
    std::vector<int32_t> hv((size_t)c->nn + 1, 0);
    if (h_off)
        for (int32_t i = 0; i < c->nn; ++i) {
            const int32_t x = c->h_perm[i];
            hv[i + 1] = hv[i] + (h_off[x + 1] - h_off[x]);
        }
    c->have_vic = false;
    if (c->voff.ensure(hv.size()) || c->vent.ensure(std::max<int32_t>(hv[c->nn], 1))) return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->voff.p, hv.data(), sizeof(int32_t) * hv.size(), hipMemcpyHostToDevice, c->st));
    if (hv[c->nn] > 0)
        HIP_TRY(launch_vic_build(c->st, off, prio, cpu, mem, gpu, c->perm.p, c->nn, c->voff.p, c->vent.p));
    HIP_TRY(hipStreamSynchronize(c->st));
    c->have_vic = true;
    return 0;
}

int check_victims_state(fit_ctx* c) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (!c->have_nodes) return fail(FIT_E_STATE, "fit_load_nodes not called");
    if (c->collective())
        return fail(FIT_E_STATE, "fit_load_victims on a sharded context (world > 1 / FIT_FLAG_COLLECTIVES)");
    return 0;
}

// --------------------------------------------------------------------------- fit_preempt_tl
// fit_preempt's sequence, classifier, slices, partials and final kernel; the
// walk reads the run lists and the timeline's own victims.
int preempt_tl_impl(fit_ctx* c, int32_t J, const JobCols& d, const int32_t* prio, fit_evict* out, int32_t* bad) {
    const int S = preempt_slices(J, c->cls_maxn, c->cus);
    if (c->pe_part.ensure(preempt_partials(J, S))) return FIT_E_OOM;
    return query_impl(
        c, J, bad,
        [&] {
            return launch_preempt_classify(c->st, c->d_ptab.p, c->np, c->ncomp, d.cpu, d.mem, d.gpu, d.wall, d.part, J,
                                           out, c->jcomp.p, bad);
        },
        [&](const ExplainComps& ec, const int32_t* jl, const int32_t* live) {
            return launch_preempt_tl(c->st, c->tlhdr.p, c->slab.p, c->vtl_span.p, c->vtl_ent.p, ec, c->tl_slots,
                                     c->tl_slot_min, c->vtl_shift, d.cpu, d.mem, d.gpu, d.wall, d.part, prio, J,
                                     c->jcomp.p, jl, live, S, c->pe_part.p, out);
        });
}

// --------------------------------------------------------------------------- fit_preempt_tl_k
// fit_preempt_k's sequence, classifier, slices, lists and final kernel; the
// walk reads the run lists and the timeline's own victims, as fit_preempt_tl's.
int preempt_tl_k_impl(fit_ctx* c, int32_t J, const JobCols& d, const int32_t* prio, int32_t kmax, fit_evict_k* out,
                      int32_t* out_node, int32_t* out_vic, int32_t* bad) {
    const int S = preempt_slices(J, c->cls_maxn, c->cus);
    if (c->pe_part.ensure(preempt_k_partials(J, S, kmax))) return FIT_E_OOM;
    return query_impl(
        c, J, bad,
        [&] {
            return launch_preempt_k_classify(c->st, c->d_ptab.p, c->np, c->ncomp, d.cpu, d.mem, d.gpu, d.wall, d.part,
                                             d.nk, kmax, J, out, out_node, out_vic, c->jcomp.p, bad);
        },
        [&](const ExplainComps& ec, const int32_t* jl, const int32_t* live) {
            return launch_preempt_tl_k(c->st, c->tlhdr.p, c->slab.p, c->vtl_span.p, c->vtl_ent.p, ec, c->tl_slots,
                                       c->tl_slot_min, c->vtl_shift, d.cpu, d.mem, d.gpu, d.wall, d.part, prio, kmax,
                                       J, c->jcomp.p, jl, live, S, c->pe_part.p, out, out_node, out_vic);
        });
}

// fit_load_victims_tl / fit_load_victims_tl_device behind their checks, as load_victims_impl: the
// position-ordered offsets from the caller's (h_off: host copy, nullptr = every list empty), then the
// entries from the device CSR.  The lists loaded before are replaced from the first write on.
int load_victims_tl_impl(fit_ctx* c, const int32_t* h_off, const int32_t* off, const int32_t* prio, const int32_t* end,
                         const int32_t* cpu, const int32_t* mem, const int32_t* gpu) {
    std::vector<VicSpan> hv((size_t)std::max(c->nn, 1), VicSpan{0, 0});
    int32_t total = 0;
    for (int32_t i = 0; i < c->nn; ++i) {
        const int32_t x = c->h_perm[i];
        hv[i] = {total, h_off ? h_off[x + 1] - h_off[x] : 0};
        total += hv[i].len;
    }
    c->have_vtl = false;
    if (c->vtl_span.ensure(hv.size()) || c->vtl_ent.ensure(std::max<int32_t>(total, 1))) return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->vtl_span.p, hv.data(), sizeof(VicSpan) * hv.size(), hipMemcpyHostToDevice, c->st));
    if (total > 0)
        HIP_TRY(launch_vtl_build(c->st, off, prio, end, cpu, mem, gpu, c->perm.p, c->nn, c->vtl_span.p, c->vtl_ent.p));
    HIP_TRY(hipStreamSynchronize(c->st));
    c->vtl_shift = 0;
    c->vtl_total = total;
    c->have_vtl = true;
    return 0;
}

int check_victims_tl_state(fit_ctx* c) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (!c->have_nodes) return fail(FIT_E_STATE, "fit_load_nodes not called");
    if (c->collective())
        return fail(FIT_E_STATE, "fit_load_victims_tl on a sharded context (world > 1 / FIT_FLAG_COLLECTIVES)");
    if (!c->have_tl) return fail(FIT_E_STATE, "fit_load_timeline not called");
    return 0;
}

// --------------------------------------------------------------------------- fit_when_k
// classify the batch, (more than a group of jobs on several components: the
// jobs in component order), then per chunk of WHENK_CHUNK jobs count (difference arrays), pick the
// start, pick the nodes, finalise.  query_impl's sequence with a chunk loop in place of its one
// walk, hence written out here.  Bounded launches on the context's stream, no
// synchronisation between chunks — the stream orders their use of the one scratch — and nothing
// waits on another workgroup.  Device pointers; *bad, the rows and the nodes are valid once the
// caller has drained the stream.
static_assert(sizeof(fit_eta_k) == 40 && offsetof(fit_eta_k, members) == 20 && offsetof(fit_eta_k, reserved) == 36,
              "fit_eta_k is 40 bytes");

// node slices per job, from the sweep of DESIGN.md §3.14: about four count workgroups (one per
// WHENK_GROUP jobs and slice) per CU from a short batch, two slices when the jobs alone fill the
// chip, and at least one workgroup's worth of nodes (256) per slice
int whenk_slices(int32_t nj, int32_t maxn, int cus) {
    const int64_t groups = ((int64_t)std::max(nj, 1) + WHENK_GROUP - 1) / WHENK_GROUP;
    const int64_t want = std::max<int64_t>(2, ((int64_t)cus * 4 + groups - 1) / groups);
    const int64_t fit = ((int64_t)maxn + 255) / 256;
    return (int)std::max<int64_t>(1, std::min<int64_t>({want, fit, (int64_t)WHENK_MAX_SLICES}));
}

// The window columns of fit_when_k_win / fit_place_tl_k_win on the device, either
// nullptr: not_before all 0, deadline none.  No WinDev at all: the unwindowed kernels.
struct WinDev {
    const int32_t *nb, *dl;
};

int when_k_impl(fit_ctx* c, int32_t J, const JobCols& d, int32_t kmax, fit_eta_k* out, int32_t* out_node,
                int32_t* bad, const WinDev* win = nullptr) {
    hipStream_t st = c->st;
    const int C = c->ncomp, H = c->tl_slots;
    const int32_t chunk = std::min<int32_t>(J, WHENK_CHUNK);
    const int S = whenk_slices(chunk, c->cls_maxn, c->cus);
    if (c->jcomp.ensure(std::max(J, 1)) || c->wk_diff.ensure((size_t)chunk * (H + 1)) ||
        c->wk_top.ensure((size_t)chunk * S * WHENK_KEYS))
        return FIT_E_OOM;
    HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int32_t), st));
    HIP_TRY(launch_whenk_classify(st, c->d_ptab.p, c->np, d.cpu, d.mem, d.gpu, d.wall, d.part, d.nk, kmax, J,
                                  c->tl_slot_min, out, out_node, c->jcomp.p, bad));
    if (C < 1) return 0;  // no node in any partition: every row is final
    // a count workgroup walks the nodes once for WHENK_GROUP jobs of one component: order the jobs
    // by component when a group would mix them
    const int32_t *jl, *live;
    if (const int rc = query_joblist(c, J, WHENK_GROUP, &jl, &live)) return rc;
    const ExplainComps ec = query_comps(c);
    for (int32_t t0 = 0; t0 < J; t0 += WHENK_CHUNK) {
        const int32_t nj = std::min<int32_t>(J - t0, WHENK_CHUNK);
        if (win)
            HIP_TRY(launch_whenk_chunk_win(st, c->tlhdr.p, c->slab.p, ec, H, c->tl_slot_min, d.cpu, d.mem, d.gpu, d.wall,
                                           d.part, t0, nj, J, kmax, c->jcomp.p, jl, live, S, c->wk_diff.p, c->wk_top.p,
                                           out, out_node, win->nb, win->dl));
        else
            HIP_TRY(launch_whenk_chunk(st, c->tlhdr.p, c->slab.p, ec, H, c->tl_slot_min, d.cpu, d.mem, d.gpu, d.wall,
                                       d.part, t0, nj, J, kmax, c->jcomp.p, jl, live, S, c->wk_diff.p, c->wk_top.p, out,
                                       out_node));
    }
    return 0;
}

// --------------------------------------------------------------------------- the timeline writers
// fit_place_tl_k, fit_unplace_tl, fit_advance_tl and fit_hold_tl follow one protocol, so that a bad
// batch writes nothing and a failed write never leaves a half-written timeline in use:
//   check phase  : ev[0], check() — launches that only read the timeline — ev[1], `flags` copied to
//                  pinned memory, ONE synchronisation; verdict() then reads the flag words: a FIT_E_*
//                  code with the call's own text fails the call, kTlNoWrite ends it with nothing to
//                  write, 0 goes on.  No `flags`: no check phase at all (fit_advance_tl without tails).
//   write phase  : ev[3], write(kept) — from its first launch on the run lists may be partly written
//                  — ev[4], `result` copied to pinned memory, the closing synchronisation.  Any HIP
//                  error in it drops the timeline (a watchdog trip of fit_place_tl does the same),
//                  unless write() set `kept` to the code of a failure that wrote nothing.
// *dev_ms: the device time of the two phases, summed.  Bounded launches on the context's stream,
// nothing waits on another workgroup: no launch lock, no watchdog.
struct TlBack {  // device words the host reads after a phase
    void* host = nullptr;
    const void* dev = nullptr;
    size_t bytes = 0;
};
constexpr int kTlNoWrite = 1;  // verdict(): the call is done, no write phase

template <class Check, class Verdict, class Write>
int tl_write_impl(fit_ctx* c, const char* name, TlBack flags, Check check, Verdict verdict, TlBack result, Write write,
                  double* dev_ms) {
    hipStream_t st = c->st;
    float ms = 0.f;
    *dev_ms = 0;
    if (flags.bytes) {
        HIP_TRY(hipEventRecord(c->ev[0], st));
        HIP_TRY(check());
        HIP_TRY(hipEventRecord(c->ev[1], st));
        HIP_TRY(hipMemcpyAsync(flags.host, flags.dev, flags.bytes, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const int rc = verdict();
        if (rc < 0) return rc;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
        *dev_ms = ms;
        if (rc == kTlNoWrite) return 0;
    }
    HIP_TRY(hipEventRecord(c->ev[3], st));
    int kept = 0;
    hipError_t e = write(kept);
    if (e != hipSuccess && kept) return kept;
    if (e == hipSuccess) e = hipEventRecord(c->ev[4], st);
    if (e == hipSuccess && result.bytes)
        e = hipMemcpyAsync(result.host, result.dev, result.bytes, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, c->ev[3], c->ev[4]);
    if (e != hipSuccess) {
        c->have_tl = false;
        return fail(FIT_E_HIP, "%s: %s; the timeline is dropped (fit_load_timeline)", name, hipGetErrorString(e));
    }
    *dev_ms += ms;
    return 0;
}

// --------------------------------------------------------------------------- fit_place_tl_k
// classify the batch and list the jobs of each component in index order
// (launch_joblists); the flag words are the bad-input flag, the reject count and the component
// offsets; then k_ptlk_commit per chunk of PTLK_CHUNK jobs of every component's list, one workgroup
// per component.  Device pointers; out (J * kmax) and outs (J) are valid on return.
int place_tl_k_impl(fit_ctx* c, int32_t J, const JobCols& d, int32_t kmax, int32_t* out, int32_t* outs,
                    fit_stats* stats, const WinDev* win = nullptr) {
    const double t0 = now_ms();
    fit_stats S;
    memset(&S, 0, sizeof S);
    S.jobs = J;
    S.engine = 4;
    const int C = c->ncomp, H = c->tl_slots;
    S.components = C;
    hipStream_t st = c->st;
    const size_t ns = 2 * ((size_t)C + 1) + 2;
    if (c->jcomp.ensure(J) || c->jl.ensure(J) || c->jpk.ensure((size_t)J + 1) ||
        c->jls.ensure(std::max<size_t>(joblists_scratch_ints(J), 1) + ns) || c->h_jls.ensure(ns) ||
        c->ptlk_cnt.ensure(1) || c->h_ptlk.ensure(1))
        return FIT_E_OOM;
    int32_t* g = c->jls.p + joblists_scratch_ints(J);  // [0] rejected, [1] bad input, then jb and mb
    int32_t* jbd = g + 2;
    int32_t maxlen = 0;          // the longest component job list
    int32_t chunk = PTLK_CHUNK;  // FIT_PTLK_CHUNK: tests put the launch seam inside a small batch
    if (const char* e = getenv("FIT_PTLK_CHUNK")) chunk = std::max(1, std::min(atoi(e), PTLK_CHUNK));
    const int rc = tl_write_impl(
        c, win ? "fit_place_tl_k_win" : "fit_place_tl_k", {c->h_jls.p, g, sizeof(int32_t) * ns},
        [&] {
            hipError_t e = launch_ptlk_classify(st, c->d_ptab.p, c->np, d.cpu, d.mem, d.gpu, d.wall, d.part, d.nk, kmax,
                                                J, out, outs, c->jcomp.p);
            if (e == hipSuccess)
                e = launch_joblists(st, c->jcomp.p, J, C, c->jls.p, g, jbd, jbd + C + 1, c->jl.p, c->jpk.p);
            return e;
        },
        [&]() -> int {
            if (c->h_jls.p[1]) return fail(FIT_E_INVAL, "a job has a negative demand or nodes_k > kmax");
            S.rejected = c->h_jls.p[0];
            for (int k = 0; k < C; ++k) maxlen = std::max(maxlen, c->h_jls.p[2 + k + 1] - c->h_jls.p[2 + k]);
            if (maxlen <= 0) return kTlNoWrite;
            HIP_TRY(hipMemsetAsync(c->ptlk_cnt.p, 0, sizeof(int32_t), st));
            return 0;
        },
        {c->h_ptlk.p, c->ptlk_cnt.p, sizeof(int32_t)},
        [&](int& kept) {
            const int threads = ptlk_threads(c->cls_maxn);
            const ExplainComps ec = query_comps(c);
            hipError_t e = hipSuccess;
            int32_t done = 0;
            for (; done < maxlen && e == hipSuccess; done += chunk)
                e = win ? launch_ptlk_commit_win(st, threads, c->tlhdr.p, c->slab.p, ec, H, c->tl_slot_min, c->jl.p, jbd,
                                                 done, chunk, d.cpu, d.mem, d.gpu, d.wall, d.part, d.nk, kmax, out, outs,
                                                 c->ptlk_cnt.p, win->nb, win->dl)
                        : launch_ptlk_commit(st, threads, c->tlhdr.p, c->slab.p, ec, H, c->tl_slot_min, c->jl.p, jbd, done,
                                             chunk, d.cpu, d.mem, d.gpu, d.wall, d.part, d.nk, kmax, out, outs,
                                             c->ptlk_cnt.p);
            if (e != hipSuccess && done <= chunk)  // the very first commit launch: nothing is reserved yet
                kept = fail(FIT_E_HIP, "k_ptlk_commit launch failed: %s", hipGetErrorString(e));
            return e;
        },
        &S.ms_device);
    if (rc) return rc;
    if (maxlen > 0) S.placed = c->h_ptlk.p[0];
    S.unplaced = J - S.placed - S.rejected;
    S.ms_total = now_ms() - t0;
    if (stats) *stats = S;
    return 0;
}

// --------------------------------------------------------------------------- fit_unplace_tl
// The rows fit_unplace_tl and fit_hold_tl take, on the device (nk: nullptr without a nodes_k column).
struct TlRows {
    const int32_t *cpu, *mem, *gpu, *wall;
    const uint16_t* nk;
    int32_t kmax;
    const int32_t *node, *start;
};

// The check phase of both: node id -> position and the check of the WHOLE batch;
// the flag words are the counters g (fit_device.h), nchunks window counts among them.
int tl_rows_ensure(fit_ctx* c, int64_t nchunks) {
    const size_t ng = 4 + (size_t)nchunks, np = std::max(c->nn, 1);
    return c->tlr_inv.ensure(std::max(c->n, 1)) || c->tlr_cnt.ensure(np) || c->tlr_first.ensure(np) ||
           c->tlr_fill.ensure(np) || c->tlr_g.ensure(ng) || c->h_tlr_g.ensure(ng);
}
TlBack tl_rows_flags(fit_ctx* c, int64_t nchunks) {
    return {c->h_tlr_g.p, c->tlr_g.p, sizeof(int32_t) * (4 + (size_t)nchunks)};
}
hipError_t tl_rows_check(fit_ctx* c, int32_t J, const TlRows& r, int32_t chunk, int64_t nchunks) {
    hipStream_t st = c->st;
    hipError_t e = hipMemsetAsync(c->tlr_g.p, 0, sizeof(int32_t) * (4 + (size_t)nchunks), st);
    if (e == hipSuccess) e = hipMemsetAsync(c->tlr_cnt.p, 0, sizeof(int32_t) * (size_t)std::max(c->nn, 1), st);
    if (e == hipSuccess) e = launch_utl_inverse(st, c->tlhdr.p, c->nn, c->n, c->tlr_inv.p);
    if (e == hipSuccess)
        e = launch_utl_check(st, r.cpu, r.mem, r.gpu, r.nk, r.kmax, r.node, r.start, J, c->n, c->tl_slots, chunk,
                             c->tlr_g.p);
    return e;
}
// the flag, and the windows of the call's live rows
int tl_rows_verdict(fit_ctx* c, int64_t nchunks, int64_t* total) {
    if (c->h_tlr_g.p[2])
        return fail(FIT_E_INVAL, "a live row has a negative demand, nodes_k > kmax, start >= %d slots, a node id "
                                 "outside [0, %d) or the same node twice", c->tl_slots, c->n);
    *total = 0;
    for (int64_t k = 0; k < nchunks; ++k) *total += c->h_tlr_g.p[4 + k];
    return 0;
}

// count, offsets, scatter and apply per chunk of UTL_CHUNK rows.  Device
// pointers; *applied (host, may be null) is valid on return.
int unplace_tl_impl(fit_ctx* c, int32_t J, const TlRows& r, int64_t* applied) {
    int32_t chunk = UTL_CHUNK;  // FIT_UTL_CHUNK: tests put the launch seam inside a small batch
    if (const char* e = getenv("FIT_UTL_CHUNK")) chunk = std::max(1, std::min(atoi(e), UTL_CHUNK));
    const int64_t nchunks = ((int64_t)J + chunk - 1) / chunk;
    const size_t wcap = (size_t)std::min(J, chunk) * r.kmax;
    if (tl_rows_ensure(c, nchunks) || c->tlr_touched.ensure(std::min<size_t>(wcap, std::max(c->nn, 1))) ||
        c->tlr_win.ensure(wcap))
        return FIT_E_OOM;
    int64_t total = 0;
    double ms = 0;
    const int rc = tl_write_impl(
        c, "fit_unplace_tl", tl_rows_flags(c, nchunks), [&] { return tl_rows_check(c, J, r, chunk, nchunks); },
        [&]() -> int {
            const int v = tl_rows_verdict(c, nchunks, &total);
            return v ? v : total > 0 && c->nn > 0 ? 0 : kTlNoWrite;
        },
        {},
        [&](int&) {
            hipError_t e = hipSuccess;
            for (int64_t k = 0; k < nchunks && e == hipSuccess; ++k) {
                const int32_t t0 = (int32_t)(k * chunk);
                e = launch_utl_chunk(c->st, c->tlhdr.p, c->slab.p, c->nn, c->tl_slots, c->tl_slot_min, r.cpu, r.mem,
                                     r.gpu, r.wall, r.nk, r.kmax, r.node, r.start, t0, std::min<int32_t>(J - t0, chunk),
                                     c->h_tlr_g.p[4 + k], c->n, c->tlr_inv.p, c->tlr_cnt.p, c->tlr_first.p,
                                     c->tlr_fill.p, c->tlr_touched.p, c->tlr_win.p, c->tlr_g.p);
            }
            return e;
        },
        &ms);
    if (rc) return rc;
    c->utl_ms = ms;
    if (applied) *applied = total;
    return 0;
}

// --------------------------------------------------------------------------- fit_advance_tl
// with tails, their check (the flag word: a tail below -1); then one launch,
// one wave per run list.  a >= 1; device pointers, n entries each, or all three null.
int advance_tl_impl(fit_ctx* c, int32_t a, const int32_t* tc, const int32_t* tm, const int32_t* tg) {
    hipStream_t st = c->st;
    if (c->atl_g.ensure(1) || c->h_atl.ensure(1)) return FIT_E_OOM;
    double ms = 0;
    const int rc = tl_write_impl(
        c, "fit_advance_tl", tc && c->n > 0 ? TlBack{c->h_atl.p, c->atl_g.p, sizeof(int32_t)} : TlBack{},
        [&] {
            const hipError_t e = hipMemsetAsync(c->atl_g.p, 0, sizeof(int32_t), st);
            return e == hipSuccess ? launch_atl_check(st, tc, tm, tg, c->n, c->atl_g.p) : e;
        },
        [&]() -> int { return c->h_atl.p[0] ? fail(FIT_E_INVAL, "a tail value is below -1") : 0; }, {},
        [&](int&) {
            return launch_atl_advance(st, c->tlhdr.p, c->slab.p, c->nn, c->n, c->tl_slots, std::min(a, c->tl_slots), tc,
                                      tm, tg);
        },
        &ms);
    if (rc) return rc;
    c->atl_ms = ms;
    // fit_preempt_tl reads every victim's end as max(end - shift, 0): no rewrite of the entries
    c->vtl_shift = std::min(c->vtl_shift + std::min(a, c->tl_slots), c->tl_slots);
    return 0;
}

// --------------------------------------------------------------------------- fit_evicted_tl
// node id -> position, then per chunk of UTL_CHUNK rows the check that marks
// the rows' entries — every chunk before the flag is read, so all positions refer to the lists as
// they were; a refused call takes its marks back and has written nothing else.  Then ONE apply launch,
// a wave per touched node.  Device pointers, m > 0.
int evicted_tl_impl(fit_ctx* c, int32_t m, const int32_t* node, const int32_t* pos) {
    hipStream_t st = c->st;
    int32_t chunk = UTL_CHUNK;  // FIT_UTL_CHUNK: tests put the launch seam inside a small batch
    if (const char* e = getenv("FIT_UTL_CHUNK")) chunk = std::max(1, std::min(atoi(e), UTL_CHUNK));
    const int32_t cap = std::min(m, c->nn);  // distinct nodes the rows can touch
    if (tl_rows_ensure(c, 0) || c->tlr_touched.ensure(std::max(cap, 1))) return FIT_E_OOM;
    double ms = 0;
    const int rc = tl_write_impl(
        c, "fit_evicted_tl", tl_rows_flags(c, 0),
        [&] {
            hipError_t e = hipMemsetAsync(c->tlr_g.p, 0, sizeof(int32_t) * 4, st);
            if (e == hipSuccess) e = hipMemsetAsync(c->tlr_cnt.p, 0, sizeof(int32_t) * (size_t)std::max(c->nn, 1), st);
            if (e == hipSuccess) e = launch_utl_inverse(st, c->tlhdr.p, c->nn, c->n, c->tlr_inv.p);
            for (int32_t t0 = 0; t0 < m && e == hipSuccess; t0 += std::min(chunk, m - t0))
                e = launch_etl_check(st, node, pos, t0, std::min(chunk, m - t0), c->n, c->tlr_inv.p, c->vtl_span.p,
                                     c->vtl_ent.p, c->tlr_cnt.p, c->tlr_touched.p, cap, c->tlr_g.p);
            return e;
        },
        [&]() -> int {
            if (!c->h_tlr_g.p[2]) return 0;
            for (int32_t t0 = 0; t0 < m; t0 += std::min(chunk, m - t0))  // the marks are scratch
                HIP_TRY(launch_etl_clear(st, node + t0, pos + t0, std::min(chunk, m - t0), c->n, c->tlr_inv.p,
                                         c->vtl_span.p, c->vtl_ent.p));
            HIP_TRY(hipStreamSynchronize(st));
            return fail(FIT_E_INVAL, "a row names a node id outside [0, %d), a position outside its node's current "
                                     "list (a node in no partition has none) or the same (node, position) twice", c->n);
        },
        {},
        [&](int&) {
            return launch_etl_apply(st, c->tlhdr.p, c->slab.p, c->tl_slots, c->vtl_shift, c->tlr_touched.p, cap,
                                    c->vtl_span.p, c->vtl_ent.p, c->tlr_g.p);
        },
        &ms);
    // a HIP error may have left marks or half-compacted lists: the lists go (fit_load_victims_tl)
    if (rc == FIT_E_HIP) c->have_vtl = false;
    if (rc) return rc;
    c->etl_ms = ms;
    return 0;
}

// --------------------------------------------------------------------------- fit_set_tl
// node id -> position and the check of the WHOLE batch (the flag words are the
// counters g: the bad-input flag, the ignored rows, the windows of every chunk), then count, offsets,
// scatter and apply per chunk of UTL_CHUNK rows.  Device pointers, m > 0; *applied and *ignored (host,
// may be null) are written on success only.
int set_tl_impl(fit_ctx* c, int32_t m, const int32_t* node, const int32_t* from, const int32_t* to, const int32_t* cpu,
                const int32_t* mem, const int32_t* gpu, int64_t* applied, int64_t* ignored) {
    hipStream_t st = c->st;
    int32_t chunk = UTL_CHUNK;  // FIT_UTL_CHUNK: tests put the launch seam inside a small batch
    if (const char* e = getenv("FIT_UTL_CHUNK")) chunk = std::max(1, std::min(atoi(e), UTL_CHUNK));
    const int64_t nchunks = ((int64_t)m + chunk - 1) / chunk;
    const size_t wcap = (size_t)std::min(m, chunk);
    if (tl_rows_ensure(c, nchunks) || c->tlr_touched.ensure(std::min<size_t>(wcap, std::max(c->nn, 1))) ||
        c->tlr_win.ensure(wcap))
        return FIT_E_OOM;
    int64_t total = 0;
    double ms = 0;
    const int rc = tl_write_impl(
        c, "fit_set_tl", tl_rows_flags(c, nchunks),
        [&] {
            hipError_t e = hipMemsetAsync(c->tlr_g.p, 0, sizeof(int32_t) * (4 + (size_t)nchunks), st);
            if (e == hipSuccess) e = hipMemsetAsync(c->tlr_cnt.p, 0, sizeof(int32_t) * (size_t)std::max(c->nn, 1), st);
            if (e == hipSuccess) e = launch_utl_inverse(st, c->tlhdr.p, c->nn, c->n, c->tlr_inv.p);
            if (e == hipSuccess)
                e = launch_stl_check(st, node, from, to, cpu, mem, gpu, m, c->n, c->tl_slots, chunk, c->tlr_inv.p,
                                     c->tlr_g.p);
            return e;
        },
        [&]() -> int {
            if (c->h_tlr_g.p[2])
                return fail(FIT_E_INVAL, "a live row has a node id outside [0, %d), from >= %d slots, to <= from or a "
                                         "level below -1", c->n, c->tl_slots);
            for (int64_t k = 0; k < nchunks; ++k) total += c->h_tlr_g.p[4 + k];
            return total > 0 && c->nn > 0 ? 0 : kTlNoWrite;
        },
        {},
        [&](int&) {
            hipError_t e = hipSuccess;
            for (int64_t k = 0; k < nchunks && e == hipSuccess; ++k) {
                const int32_t t0 = (int32_t)(k * chunk);
                e = launch_stl_chunk(st, c->tlhdr.p, c->slab.p, c->nn, c->tl_slots, node, from, to, cpu, mem, gpu, t0,
                                     std::min<int32_t>(m - t0, chunk), c->h_tlr_g.p[4 + k], c->n, c->tlr_inv.p,
                                     c->tlr_cnt.p, c->tlr_first.p, c->tlr_fill.p, c->tlr_touched.p, c->tlr_win.p,
                                     c->tlr_g.p);
            }
            return e;
        },
        &ms);
    if (rc) return rc;
    const int64_t ign = c->h_tlr_g.p[3];
    if (total + ign > 0) c->stl_ms = ms;  // a call with a live row
    if (applied) *applied = total;
    if (ignored) *ignored = ign;
    return 0;
}

// --------------------------------------------------------------------------- fit_hold_tl
// fit_unplace_tl's rows and check phase — nothing, out_state included, is
// written before the flag is seen — then the windows of the whole call grouped by node, the judge
// pass, the apply pass and the states with the two counts.  Device pointers; *applied and *refused
// (host, may be null) are valid on return.
int hold_tl_impl(fit_ctx* c, int32_t J, const TlRows& r, int32_t* out_state, int64_t* applied, int64_t* refused) {
    hipStream_t st = c->st;
    const int64_t nchunks = ((int64_t)J + UTL_CHUNK - 1) / UTL_CHUNK;  // of the check's window counts only
    if (tl_rows_ensure(c, nchunks) || c->tlr_flag.ensure(J) || c->tlr_tot.ensure(2) || c->h_tlr_tot.ensure(2))
        return FIT_E_OOM;
    int64_t total = 0;
    double ms = 0;
    const int rc = tl_write_impl(
        c, "fit_hold_tl", tl_rows_flags(c, nchunks),
        [&] {
            hipError_t e = hipMemsetAsync(c->tlr_flag.p, 0, sizeof(int32_t) * (size_t)J, st);
            if (e == hipSuccess) e = hipMemsetAsync(c->tlr_tot.p, 0, sizeof(unsigned long long) * 2, st);
            return e == hipSuccess ? tl_rows_check(c, J, r, UTL_CHUNK, nchunks) : e;
        },
        [&]() -> int {
            const int v = tl_rows_verdict(c, nchunks, &total);
            if (v) return v;
            if (total > INT32_MAX) return fail(FIT_E_OOM, "%lld windows in one call", (long long)total);
            if (c->tlr_win.ensure((size_t)std::max<int64_t>(total, 1)) ||
                c->tlr_touched.ensure((size_t)std::max<int64_t>(std::min<int64_t>(total, c->nn), 1)))
                return FIT_E_OOM;
            return 0;
        },
        {c->h_tlr_tot.p, c->tlr_tot.p, sizeof(unsigned long long) * 2},
        [&](int&) {
            hipError_t e = launch_htl_hold(st, c->tlhdr.p, c->slab.p, c->nn, c->tl_slots, c->tl_slot_min, r.cpu, r.mem,
                                           r.gpu, r.wall, r.nk, r.kmax, r.node, r.start, J, (int32_t)total, c->n,
                                           c->tlr_inv.p, c->tlr_cnt.p, c->tlr_first.p, c->tlr_fill.p, c->tlr_touched.p,
                                           c->tlr_win.p, c->tlr_flag.p, c->tlr_g.p);
            if (e == hipSuccess)
                e = launch_htl_final(st, r.nk, r.kmax, r.start, J, c->tlr_flag.p, out_state, c->tlr_tot.p);
            return e;
        },
        &ms);
    if (rc) return rc;
    c->htl_ms = ms;
    if (applied) *applied = (int64_t)c->h_tlr_tot.p[0];
    if (refused) *refused = (int64_t)c->h_tlr_tot.p[1];
    return 0;
}

// The tests every entry point that takes a job batch makes, in the order its callers see them.
// query: the entry point's name for fit_explain / fit_when (they also refuse j < 0 first and a
// sharded context), nullptr for the placements.  tl: 1 a timeline must be loaded, -1 none may be.
int check_job_args(fit_ctx* c, int32_t j, std::initializer_list<const void*> arrays, const char* query, int tl) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (query && j < 0) return fail(FIT_E_INVAL, "j=%d", j);
    if (!c->have_nodes) return fail(FIT_E_STATE, "fit_load_nodes not called");
    if (query && c->collective())
        return fail(FIT_E_STATE, "%s on a sharded context (world > 1 / FIT_FLAG_COLLECTIVES)", query);
    if (tl < 0 && c->have_tl) return fail(FIT_E_STATE, "%s while a timeline is loaded", query);
    if (tl > 0 && !c->have_tl) return fail(FIT_E_STATE, "fit_load_timeline not called");
    if (j < 0 || (j > 0 && std::find(arrays.begin(), arrays.end(), nullptr) != arrays.end()))
        return fail(FIT_E_INVAL, "bad job arrays");
    return 0;
}

// fit_place, fit_explain, fit_when: the batch's columns packed in pinned memory and sent in ONE
// copy (the previous call's copy is complete: each of them ends with a synchronisation).  Four
// int32 columns, then part and, if given, nodes_k, each rounded up to 4 bytes.
int stage_packed(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                 const int32_t* wall, const uint16_t* part, const uint16_t* nk, JobCols& d) {
    const size_t b = sizeof(int32_t) * j, bh = sizeof(uint16_t) * j, bh4 = (bh + 3) & ~(size_t)3;
    const size_t tot = 4 * b + 2 * bh4;
    if (c->jpack.ensure(tot) || c->h_jpack.ensure(tot)) return FIT_E_OOM;
    uint8_t* h = c->h_jpack.p;
    memcpy(h, cpu, b);
    memcpy(h + b, mem, b);
    memcpy(h + 2 * b, gpu, b);
    memcpy(h + 3 * b, wall, b);
    memcpy(h + 4 * b, part, bh);
    if (nk) memcpy(h + 4 * b + bh4, nk, bh);
    HIP_TRY(hipMemcpyAsync(c->jpack.p, h, nk ? tot : 4 * b + bh4, hipMemcpyHostToDevice, c->st));
    const uint8_t* p = c->jpack.p;
    d = {(const int32_t*)p, (const int32_t*)(p + b), (const int32_t*)(p + 2 * b), (const int32_t*)(p + 3 * b),
         (const uint16_t*)(p + 4 * b), nk ? (const uint16_t*)(p + 4 * b + bh4) : nullptr};
    return 0;
}

// fit_place above kPackJobs and fit_place_tl: one copy per column into the context's job columns
// (has_nk: the entry point has a nodes_k column at all).
int stage_columns(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                  const int32_t* wall, const uint16_t* part, bool has_nk, const uint16_t* nk, JobCols& d) {
    const size_t m = std::max(j, 1), b = sizeof(int32_t) * j, bh = sizeof(uint16_t) * j;
    if (c->jcpu.ensure(m) || c->jmem.ensure(m) || c->jgpu.ensure(m) || c->jwall.ensure(m) ||
        c->jpart.ensure(m) || (has_nk && c->jk.ensure(m)))
        return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->jcpu.p, cpu, b, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->jmem.p, mem, b, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->jgpu.p, gpu, b, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->jwall.p, wall, b, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->jpart.p, part, bh, hipMemcpyHostToDevice, c->st));
    if (nk) HIP_TRY(hipMemcpyAsync(c->jk.p, nk, bh, hipMemcpyHostToDevice, c->st));
    d = {c->jcpu.p, c->jmem.p, c->jgpu.p, c->jwall.p, c->jpart.p, nk ? c->jk.p : nullptr};
    return 0;
}

// fit_explain / fit_when from host memory: the columns in one copy, impl(columns, rows, flag) with
// the flag word behind the rows so that rows and flag come back in ONE copy, a spinning wait for a
// batch of k_small's size, the flag test (bad(): the entry point's error) and the rows out.
template <class Row, class Impl, class Bad>
int query_host(fit_ctx* c, QueryBufs<Row>& Q, int32_t j, const int32_t* cpu, const int32_t* mem,
               const int32_t* gpu, const int32_t* wall, const uint16_t* part, const uint16_t* nk, Row* out,
               Impl impl, Bad bad) {
    HIP_TRY(hipSetDevice(c->device));
    JobCols d;
    int rc = stage_packed(c, j, cpu, mem, gpu, wall, part, nk, d);
    if (rc) return rc;
    if (Q.out.ensure((size_t)j + 1) || Q.h.ensure((size_t)j + 1)) return FIT_E_OOM;
    rc = impl(c, j, d, Q.out.p, reinterpret_cast<int32_t*>(Q.out.p + j));
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(Q.h.p, Q.out.p, sizeof(Row) * ((size_t)j + 1), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(j <= SMALL_ARGJ ? sync_small(c) : hipStreamSynchronize(c->st));
    if (Q.h.p[j].code) return bad();
    memcpy(out, Q.h.p, sizeof(Row) * j);
    return 0;
}

// The same on device columns and rows: only the flag word comes back, and an event pair around the
// launches gives the device time (Q.ms).
template <class Row, class Impl, class Bad>
int query_device(fit_ctx* c, QueryBufs<Row>& Q, int32_t j, const JobCols& d, Row* out, Impl impl, Bad bad) {
    HIP_TRY(hipSetDevice(c->device));
    if (Q.bad.ensure(1) || Q.h.ensure(1)) return FIT_E_OOM;
    HIP_TRY(hipEventRecord(c->ev[0], c->st));
    const int rc = impl(c, j, d, out, Q.bad.p);
    if (rc) return rc;
    HIP_TRY(hipEventRecord(c->ev[1], c->st));
    HIP_TRY(hipMemcpyAsync(Q.h.p, Q.bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    if (Q.h.p[0].code) return bad();
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    Q.ms = ms;
    return 0;
}

int bad_explain_job() { return fail(FIT_E_INVAL, "a job has a negative demand or nodes_k > %d", FIT_MAX_K); }
int bad_when_job() { return fail(FIT_E_INVAL, "a job has a negative demand"); }
int bad_room_job() { return fail(FIT_E_INVAL, "a job has a negative demand"); }

int load_timeline_impl(fit_ctx* c, int32_t slots, int32_t slot_min, int64_t ne) {
    if (c->tlhdr.ensure(std::max(c->nn, 1)) ||
        c->slab.ensure((size_t)std::max(c->nn, 1) * TL_MAX_SLOTS) || c->tl_err.ensure(1) ||
        c->h_tl_err.ensure(1))
        return FIT_E_OOM;
    c->have_vtl = false;  // the victims' ends are slots of the timeline they were loaded for
    HIP_TRY(hipMemsetAsync(c->tl_err.p, 0, 4, c->st));
    HIP_TRY(launch_build_tl(c->st, c->col_cpu.p, c->col_mem.p, c->col_gpu.p, c->col_av.p,
                            c->col_mask.p, c->perm.p, c->nn, slots, slot_min, ne >= 0 ? c->rel_off.p : nullptr,
                            c->rel_slot.p, c->rel_cpu.p, c->rel_mem.p, c->rel_gpu.p, c->slab.p,
                            c->tlhdr.p, c->tl_err.p));
    HIP_TRY(hipMemcpyAsync(c->h_tl_err.p, c->tl_err.p, 4, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    if (c->h_tl_err.p[0])
        return fail(FIT_E_INVAL, "release events: slots must be non-decreasing per node and "
                                 "amounts >= 0");
    c->tl_slots = slots;
    c->tl_slot_min = slot_min;
    c->have_tl = true;
    return 0;
}

int check_timeline_args(fit_ctx* c, int32_t slots, int32_t slot_min) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (!c->have_nodes) return fail(FIT_E_STATE, "fit_load_nodes not called");
    if (slots < 1 || slots > TL_MAX_SLOTS || slot_min < 1)
        return fail(FIT_E_INVAL, "horizon of %d slots x %d min (1..%d slots)", slots, slot_min,
                    TL_MAX_SLOTS);
    // positions stop one short of the field's range: start 1023, an all-capped score and position
    // 2^22 - 1 would make a feasible key equal to KEY_INF ("no start")
    if (c->nn > (int32_t)TL_POS_MASK)
        return fail(FIT_E_INVAL, "%d nodes: the timeline key's %d-bit position holds at most %d", c->nn,
                    TL_POS_BITS, (int32_t)TL_POS_MASK);
    return 0;
}

}  // namespace

// ============================================================================ C-ABI
extern "C" {

int fit_abi_version(void) { return FITGPU_ABI_VERSION; }

int fit_lock_dir(char* buf, int32_t buflen) {
    std::string dir;
    const int shared = resolve_lock_dir(dir);
    if (!buf || buflen <= (int32_t)dir.size()) return fail(FIT_E_INVAL, "fit_lock_dir: buffer too small");
    memcpy(buf, dir.c_str(), dir.size() + 1);
    return shared;
}

const char* fit_strerror(int code) {
    switch (code) {
        case FIT_OK: return "ok";
        case FIT_E_INVAL: return "invalid argument";
        case FIT_E_HIP: return "HIP runtime error";
        case FIT_E_RCCL: return "RCCL error";
        case FIT_E_OOM: return "out of memory";
        case FIT_E_NODEV: return "no usable gfx950 device";
        case FIT_E_STATE: return "call out of order";
        case FIT_E_PARSE: return "parse error";
        case FIT_E_UNLIMITED: return "duration is unlimited";
        default: return "unknown error";
    }
}

const char* fit_last_error(void) { return g_last_error.c_str(); }

int fit_nccl_unique_id(void* out128) {
    if (!out128) return fail(FIT_E_INVAL, "null id buffer");
    ncclUniqueId id;
    NCCL_TRY(ncclGetUniqueId(&id));
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    memcpy(out128, &id, sizeof id);
    return 0;
}

int fit_create(const fit_opts* opts, fit_ctx** out_ctx) {
    if (!out_ctx) return fail(FIT_E_INVAL, "null out_ctx");
    *out_ctx = nullptr;
    fit_opts o;
    memset(&o, 0, sizeof o);
    o.device = -1;
    o.world = 1;
    if (opts) o = *opts;
    if (o.world < 1 || o.rank < 0 || o.rank >= o.world)
        return fail(FIT_E_INVAL, "rank %d / world %d", o.rank, o.world);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail(FIT_E_NODEV, "no HIP device visible");
    int dev = o.device;
    if (dev < 0 && hipGetDevice(&dev) != hipSuccess) dev = 0;
    if (dev >= ndev) return fail(FIT_E_INVAL, "device %d of %d", dev, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(FIT_E_NODEV, "device %d is %s, this build targets gfx950", dev,
                    prop.gcnArchName);
    HIP_TRY(hipSetDevice(dev));
    fit_ctx* c = new (std::nothrow) fit_ctx();
    if (!c) return fail(FIT_E_OOM, "context allocation");
    c->device = dev;
    c->cus = prop.multiProcessorCount;
    if (const char* ev = getenv("FIT_WATCHDOG_MS"))
        c->wd_ticks = (unsigned)std::min<double>(4.29e9, std::max(1.0, atof(ev) * 1e5));
    // unset FIT_ENGINE: k_small up to small_direct jobs, the host-driven rounds up to small_batch
    // live jobs, the persistent engine above (FIT_SMALL_DIRECT, FIT_SMALL_BATCH)
    if (const char* ev = getenv("FIT_SMALL_BATCH")) c->small_batch = atoi(ev);
    if (const char* ev = getenv("FIT_SMALL_DIRECT")) c->small_direct = atoi(ev);
    if (const char* ev = getenv("FIT_SMALL_ARGS")) c->small_args = atoi(ev) != 0;
    if (const char* ev = getenv("FIT_SYNC_SPIN")) c->sync_spin = atoi(ev) != 0;
    // FIT_ENGINE forces one engine at every size: "rounds", "persistent" or "direct" (k_small)
    if (const char* ev = getenv("FIT_CLASS")) c->cls_mode = atoi(ev) ? 1 : 0;  // unset: automatic (3)
    if (const char* ev = getenv("FIT_ENGINE")) {
        c->persistent = strcmp(ev, "rounds") != 0;
        if (strcmp(ev, "persistent") == 0 || strcmp(ev, "class") == 0) c->small_batch = -1;
        c->small_direct = strcmp(ev, "direct") == 0 ? INT32_MAX : -1;
        c->cls_mode = strcmp(ev, "class") == 0 ? 2 : 0;
    }
    c->rank = o.rank;
    c->world = o.world;
    c->force_coll = (o.flags & FIT_FLAG_COLLECTIVES) != 0;
    c->shard_mode = o.shard_mode;
    c->xchg = o.exchange;
    c->xchg_user = o.exchange_user;
    if (o.window_min > 0) c->wmin = o.window_min;
    if (o.window_max > 0) c->wmax = std::max(o.window_max, c->wmin);
    for (int p = 0; p < 32; ++p) {
        c->comp_of_part[p] = -1;
        c->ptab[p] = c->ptab[32 + p] = c->ptab[64 + p] = -1;
        c->ptab[96 + p] = -1;
    }
    int rc = 0;
    if (hipStreamCreateWithFlags(&c->st, hipStreamNonBlocking) != hipSuccess) rc = FIT_E_HIP;
    for (auto& e : c->ev)
        if (!rc && hipEventCreate(&e) != hipSuccess) rc = FIT_E_HIP;
    if (!rc && c->world == 1 && c->force_coll && !c->xchg) {
        // FIT_FLAG_COLLECTIVES: a one-rank RCCL communicator, so the sharded code path and its
        // RCCL calls run on one GPU exactly as they do in a multi-GPU group
        ncclUniqueId id;
        ncclResult_t r = ncclGetUniqueId(&id);
        if (r == ncclSuccess) r = ncclCommInitRank(&c->comm, 1, id, 0);
        if (r != ncclSuccess) rc = fail(FIT_E_RCCL, "ncclCommInitRank(1 rank): %s", ncclGetErrorString(r));
    } else if (!rc && c->world > 1 && !c->xchg) {
        if (!o.nccl_id) {
            rc = fail(FIT_E_INVAL, "world > 1 needs nccl_id");
        } else {
            ncclUniqueId id;
            memcpy(&id, o.nccl_id, sizeof id);
            ncclResult_t r = ncclCommInitRank(&c->comm, c->world, id, c->rank);
            if (r != ncclSuccess)
                rc = fail(FIT_E_RCCL, "ncclCommInitRank: %s", ncclGetErrorString(r));
        }
    } else if (rc) {
        fail(rc, "stream/event creation failed");
    }
    if (rc) {
        delete c;
        return rc;
    }
    *out_ctx = c;
    return 0;
}

int fit_set_watchdog_us(fit_ctx* c, int64_t us) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (us <= 0) {
        c->wd_ticks = 1000000000u;
        if (const char* ev = getenv("FIT_WATCHDOG_MS"))
            c->wd_ticks = (unsigned)std::min<double>(4.29e9, std::max(1.0, atof(ev) * 1e5));
        return 0;
    }
    // 100 realtime ticks per microsecond; the ticks are a 32-bit kernel argument (<= 42.9 s)
    c->wd_ticks = (unsigned)std::min<int64_t>(us * 100, 4290000000ll);
    return 0;
}

void fit_destroy(fit_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->st);
    delete ctx;
}

// fit_load_nodes / fit_load_nodes_device: the argument test and the five columns into col_*.
static int load_node_cols(fit_ctx* c, int32_t n, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                          const int32_t* av, const uint32_t* mask, hipMemcpyKind kind) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (n < 0 || n > FIT_MAX_NODES || (n > 0 && (!cpu || !mem || !gpu || !av || !mask)))
        return fail(FIT_E_INVAL, "bad node arrays");
    // the columns are overwritten below: until the load succeeds there is no valid node table
    // (a failed load must not leave new offsets paired with old node rows)
    c->have_nodes = c->have_tl = false;
    c->have_vic = c->have_vtl = false;  // the victims are lists by node id, and the ids change
    HIP_TRY(hipSetDevice(c->device));
    if (alloc_cols(c, n)) return FIT_E_OOM;
    const size_t b = sizeof(int32_t) * n;
    HIP_TRY(hipMemcpyAsync(c->col_cpu.p, cpu, b, kind, c->st));
    HIP_TRY(hipMemcpyAsync(c->col_mem.p, mem, b, kind, c->st));
    HIP_TRY(hipMemcpyAsync(c->col_gpu.p, gpu, b, kind, c->st));
    HIP_TRY(hipMemcpyAsync(c->col_av.p, av, b, kind, c->st));
    HIP_TRY(hipMemcpyAsync(c->col_mask.p, mask, b, kind, c->st));
    return 0;
}

int fit_load_nodes(fit_ctx* c, int32_t n, const int32_t* cpu, const int32_t* mem,
                   const int32_t* gpu, const int32_t* av, const uint32_t* mask) {
    const int rc = load_node_cols(c, n, cpu, mem, gpu, av, mask, hipMemcpyHostToDevice);
    if (rc) return rc;
    c->h_mask.assign(mask, mask + n);
    return load_nodes_common(c, n);
}

int fit_load_nodes_device(fit_ctx* c, int32_t n, const int32_t* cpu, const int32_t* mem,
                          const int32_t* gpu, const int32_t* av, const uint32_t* mask) {
    const int rc = load_node_cols(c, n, cpu, mem, gpu, av, mask, hipMemcpyDeviceToDevice);
    if (rc) return rc;
    c->h_mask.resize(n);
    HIP_TRY(hipMemcpyAsync(c->h_mask.data(), mask, sizeof(uint32_t) * n, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return load_nodes_common(c, n);
}

int fit_load_partitions(fit_ctx* c, int32_t p, const int32_t* max_time,
                        const int32_t* max_cpus, const int32_t* max_mem) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (p < 0 || p > FIT_MAX_PARTITIONS || (p > 0 && (!max_time || !max_cpus || !max_mem)))
        return fail(FIT_E_INVAL, "bad partition table (p=%d)", p);
    HIP_TRY(hipSetDevice(c->device));
    c->np = p;
    for (int i = 0; i < 32; ++i) {
        c->ptab[i] = i < p ? max_time[i] : -1;
        c->ptab[32 + i] = i < p ? max_cpus[i] : -1;
        c->ptab[64 + i] = i < p ? max_mem[i] : -1;
    }
    int rc = build_ptab(c);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));
    return 0;
}

static int check_place_args(fit_ctx* c, int32_t j, std::initializer_list<const void*> arrays, int32_t kmax) {
    const int rc = check_job_args(c, j, arrays, nullptr, 0);
    if (rc) return rc;
    if (kmax < 1 || kmax > FIT_MAX_K)
        return fail(FIT_E_INVAL, "kmax=%d outside [1, %d]", kmax, FIT_MAX_K);
    return 0;
}

// fit_place copies a batch of at most this many jobs as one packed transfer
constexpr int32_t kPackJobs = 16384;

int fit_place(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
              const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax,
              int32_t* out, fit_stats* stats) {
    int rc = check_place_args(c, j, {cpu, mem, gpu, wall, part, out}, kmax);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // demands >= 0 and nodes_k <= kmax are checked on the device (k_prefilter): FIT_E_INVAL
    size_t m = std::max(j, 1);
    // the out buffer's tail holds the direct placement's stats (place_direct: one copy back)
    if (c->out.ensure(m * kmax + 2 + FIT_MAX_PARTITIONS + 1)) return FIT_E_OOM;
    if (c->small_args && j <= SMALL_ARGJ && j <= c->small_direct && !c->collective()) {
        // the batch in k_small's kernel arguments: no copy to the device at all
        SmallBatch hb;
        memcpy(hb.cpu, cpu, sizeof(int32_t) * j);
        memcpy(hb.mem, mem, sizeof(int32_t) * j);
        memcpy(hb.gpu, gpu, sizeof(int32_t) * j);
        memcpy(hb.wall, wall, sizeof(int32_t) * j);
        memcpy(hb.part, part, sizeof(uint16_t) * j);
        if (nk) memcpy(hb.nk, nk, sizeof(uint16_t) * j);
        bool done = false;
        rc = place_impl(c, j, nullptr, nullptr, nullptr, nullptr, nullptr, nk, kmax, c->out.p, stats, out, &done,
                        &hb);
        if (rc) return rc;
        if (!done) return fail(FIT_E_HIP, "direct placement did not return its placements");
        return 0;
    }
    // up to kPackJobs jobs (admission): the columns in ONE copy; above, one copy per column
    JobCols d;
    rc = j <= kPackJobs ? stage_packed(c, j, cpu, mem, gpu, wall, part, nk, d)
                        : stage_columns(c, j, cpu, mem, gpu, wall, part, true, nk, d);
    if (rc) return rc;
    bool done = false;
    rc = place_impl(c, j, d.cpu, d.mem, d.gpu, d.wall, d.part, d.nk, kmax, c->out.p, stats, out, &done);
    if (rc) return rc;
    if (done) return 0;  // the direct small placement copied the placements back with its stats
    HIP_TRY(hipMemcpyAsync(out, c->out.p, sizeof(int32_t) * j * kmax, hipMemcpyDeviceToHost,
                           c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return 0;
}

int fit_place_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem,
                     const int32_t* gpu, const int32_t* wall, const uint16_t* part,
                     const uint16_t* nk, int32_t kmax, int32_t* out, fit_stats* stats) {
    int rc = check_place_args(c, j, {cpu, mem, gpu, wall, part, out}, kmax);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    rc = place_impl(c, j, cpu, mem, gpu, wall, part, nk, kmax, out, stats);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));
    return 0;
}

int fit_explain(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                const int32_t* wall, const uint16_t* part, const uint16_t* nk, fit_why* out) {
    const int rc = check_job_args(c, j, {cpu, mem, gpu, wall, part, out}, "fit_explain", -1);
    if (rc || j == 0) return rc;
    return query_host(c, c->ex, j, cpu, mem, gpu, wall, part, nk, out, explain_impl, bad_explain_job);
}

int fit_explain_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                       const int32_t* wall, const uint16_t* part, const uint16_t* nk, fit_why* out) {
    const int rc = check_job_args(c, j, {cpu, mem, gpu, wall, part, out}, "fit_explain", -1);
    if (rc || j == 0) return rc;
    return query_device(c, c->ex, j, {cpu, mem, gpu, wall, part, nk}, out, explain_impl, bad_explain_job);
}

int fit_explain_ms(fit_ctx* c, double* ms) {
    if (!c || !ms) return fail(FIT_E_INVAL, "null argument");
    if (c->ex.ms < 0) return fail(FIT_E_STATE, "no fit_explain_device yet");
    *ms = c->ex.ms;
    return 0;
}

int fit_when(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
             const int32_t* wall, const uint16_t* part, fit_eta* out) {
    const int rc = check_job_args(c, j, {cpu, mem, gpu, wall, part, out}, "fit_when", 1);
    if (rc || j == 0) return rc;
    return query_host(c, c->wh, j, cpu, mem, gpu, wall, part, nullptr, out, when_impl, bad_when_job);
}

int fit_when_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                    const int32_t* wall, const uint16_t* part, fit_eta* out) {
    const int rc = check_job_args(c, j, {cpu, mem, gpu, wall, part, out}, "fit_when", 1);
    if (rc || j == 0) return rc;
    return query_device(c, c->wh, j, {cpu, mem, gpu, wall, part, nullptr}, out, when_impl, bad_when_job);
}

int fit_when_ms(fit_ctx* c, double* ms) {
    if (!c || !ms) return fail(FIT_E_INVAL, "null argument");
    if (c->wh.ms < 0) return fail(FIT_E_STATE, "no fit_when_device yet");
    *ms = c->wh.ms;
    return 0;
}

// fit_when_k / fit_when_k_device: fit_when's tests, then kmax (nodes_k against kmax is the
// device's flag word)
static int check_when_k_args(fit_ctx* c, int32_t j, std::initializer_list<const void*> arrays, int32_t kmax,
                             const char* name = "fit_when_k") {
    const int rc = check_job_args(c, j, arrays, name, 1);
    if (rc) return rc;
    if (kmax < 1 || kmax > FIT_MAX_K) return fail(FIT_E_INVAL, "kmax=%d (1..%d)", kmax, FIT_MAX_K);
    return 0;
}

static int bad_when_k_job() { return fail(FIT_E_INVAL, "a job has a negative demand or nodes_k > kmax"); }

int fit_when_k(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
               const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax, fit_eta_k* out,
               int32_t* out_node) {
    const int rc = check_when_k_args(c, j, {cpu, mem, gpu, wall, part, out, out_node}, kmax);
    if (rc || j == 0) return rc;
    // the node lists come back into pinned memory behind the launches, ahead of query_host's copy of
    // the rows and its synchronisation; they reach out_node only when the call succeeds
    const size_t nn = (size_t)j * kmax;
    if (c->wk_node.ensure(nn) || c->h_wk_node.ensure(nn)) return FIT_E_OOM;
    const int r = query_host(
        c, c->wk, j, cpu, mem, gpu, wall, part, nk, out,
        [&](fit_ctx* x, int32_t n, const JobCols& d, fit_eta_k* rows, int32_t* bad) {
            const int e = when_k_impl(x, n, d, kmax, rows, x->wk_node.p, bad);
            if (e) return e;
            HIP_TRY(hipMemcpyAsync(x->h_wk_node.p, x->wk_node.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, x->st));
            return 0;
        },
        bad_when_k_job);
    if (r) return r;
    memcpy(out_node, c->h_wk_node.p, sizeof(int32_t) * nn);
    return 0;
}

int fit_when_k_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                      const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax, fit_eta_k* out,
                      int32_t* out_node) {
    const int rc = check_when_k_args(c, j, {cpu, mem, gpu, wall, part, out, out_node}, kmax);
    if (rc || j == 0) return rc;
    return query_device(
        c, c->wk, j, {cpu, mem, gpu, wall, part, nk}, out,
        [&](fit_ctx* x, int32_t n, const JobCols& d, fit_eta_k* rows, int32_t* bad) {
            return when_k_impl(x, n, d, kmax, rows, out_node, bad);
        },
        bad_when_k_job);
}

int fit_when_k_ms(fit_ctx* c, double* ms) {
    if (!c || !ms) return fail(FIT_E_INVAL, "null argument");
    if (c->wk.ms < 0) return fail(FIT_E_STATE, "no fit_when_k_device yet");
    *ms = c->wk.ms;
    return 0;
}

// fit_when_k_win / fit_place_tl_k_win: the optional window columns of a host entry point, one copy
// each into the context's own columns (j > 0); a NULL column stays NULL
static int stage_window(fit_ctx* c, int32_t j, const int32_t* not_before, const int32_t* deadline, WinDev& w) {
    const size_t b = sizeof(int32_t) * (size_t)j;
    if ((not_before && c->win_nb.ensure(j)) || (deadline && c->win_dl.ensure(j))) return FIT_E_OOM;
    if (not_before) HIP_TRY(hipMemcpyAsync(c->win_nb.p, not_before, b, hipMemcpyHostToDevice, c->st));
    if (deadline) HIP_TRY(hipMemcpyAsync(c->win_dl.p, deadline, b, hipMemcpyHostToDevice, c->st));
    w = {not_before ? c->win_nb.p : nullptr, deadline ? c->win_dl.p : nullptr};
    return 0;
}

int fit_when_k_win(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                   const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax,
                   const int32_t* not_before, const int32_t* deadline, fit_eta_k* out, int32_t* out_node) {
    const int rc = check_when_k_args(c, j, {cpu, mem, gpu, wall, part, out, out_node}, kmax, "fit_when_k_win");
    if (rc || j == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t nn = (size_t)j * kmax;
    if (c->wk_node.ensure(nn) || c->h_wk_node.ensure(nn)) return FIT_E_OOM;
    WinDev w;
    if (const int e = stage_window(c, j, not_before, deadline, w)) return e;
    const int r = query_host(
        c, c->wkw, j, cpu, mem, gpu, wall, part, nk, out,
        [&](fit_ctx* x, int32_t n, const JobCols& d, fit_eta_k* rows, int32_t* bad) {
            const int e = when_k_impl(x, n, d, kmax, rows, x->wk_node.p, bad, &w);
            if (e) return e;
            HIP_TRY(hipMemcpyAsync(x->h_wk_node.p, x->wk_node.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, x->st));
            return 0;
        },
        bad_when_k_job);
    if (r) return r;
    memcpy(out_node, c->h_wk_node.p, sizeof(int32_t) * nn);
    return 0;
}

int fit_when_k_win_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                          const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax,
                          const int32_t* not_before, const int32_t* deadline, fit_eta_k* out, int32_t* out_node) {
    const int rc = check_when_k_args(c, j, {cpu, mem, gpu, wall, part, out, out_node}, kmax, "fit_when_k_win");
    if (rc || j == 0) return rc;
    const WinDev w{not_before, deadline};
    return query_device(
        c, c->wkw, j, {cpu, mem, gpu, wall, part, nk}, out,
        [&](fit_ctx* x, int32_t n, const JobCols& d, fit_eta_k* rows, int32_t* bad) {
            return when_k_impl(x, n, d, kmax, rows, out_node, bad, &w);
        },
        bad_when_k_job);
}

int fit_when_k_win_ms(fit_ctx* c, double* ms) {
    if (!c || !ms) return fail(FIT_E_INVAL, "null argument");
    if (c->wkw.ms < 0) return fail(FIT_E_STATE, "no fit_when_k_win_device yet");
    *ms = c->wkw.ms;
    return 0;
}

int fit_room(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu, const int32_t* wall,
             const uint16_t* part, struct fit_room* out) {
    const int rc = check_job_args(c, j, {cpu, mem, gpu, wall, part, out}, "fit_room", -1);
    if (rc || j == 0) return rc;
    return query_host(c, c->rm, j, cpu, mem, gpu, wall, part, nullptr, out, room_impl, bad_room_job);
}

int fit_room_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                    const int32_t* wall, const uint16_t* part, struct fit_room* out) {
    const int rc = check_job_args(c, j, {cpu, mem, gpu, wall, part, out}, "fit_room", -1);
    if (rc || j == 0) return rc;
    return query_device(c, c->rm, j, {cpu, mem, gpu, wall, part, nullptr}, out, room_impl, bad_room_job);
}

int fit_room_ms(fit_ctx* c, double* ms) {
    if (!c || !ms) return fail(FIT_E_INVAL, "null argument");
    if (c->rm.ms < 0) return fail(FIT_E_STATE, "no fit_room_device yet");
    *ms = c->rm.ms;
    return 0;
}

int fit_load_victims(fit_ctx* c, const int32_t* vic_off, const int32_t* vic_prio, const int32_t* vic_cpu,
                     const int32_t* vic_mem, const int32_t* vic_gpu) {
    const int rc = check_victims_state(c);
    if (rc) return rc;
    int64_t nv = 0;
    if (vic_off) {  // everything is judged before anything is written: a bad list leaves the loaded victims
        if (vic_off[0] != 0) return fail(FIT_E_INVAL, "vic_off[0] must be 0");
        for (int32_t x = 0; x < c->n; ++x)
            if (vic_off[x + 1] < vic_off[x]) return fail(FIT_E_INVAL, "vic_off decreases at %d", x);
        nv = vic_off[c->n];
        if (nv > 0 && (!vic_prio || !vic_cpu || !vic_mem || !vic_gpu)) return fail(FIT_E_INVAL, "null victim arrays");
        for (int32_t x = 0; x < c->n; ++x)
            for (int32_t k = vic_off[x]; k < vic_off[x + 1]; ++k) {
                if (vic_cpu[k] < 0 || vic_mem[k] < 0 || vic_gpu[k] < 0)
                    return fail(FIT_E_INVAL, "victim %d of node %d holds a negative amount", k - vic_off[x], x);
                if (k > vic_off[x] && vic_prio[k] < vic_prio[k - 1])
                    return fail(FIT_E_INVAL, "victims of node %d are not in eviction order (priority decreases at %d)",
                                x, k - vic_off[x]);
            }
    }
    HIP_TRY(hipSetDevice(c->device));
    if (nv > 0) {
        const size_t b = sizeof(int32_t) * nv, bo = sizeof(int32_t) * ((size_t)c->n + 1);
        if (c->vs_off.ensure((size_t)c->n + 1) || c->vs_prio.ensure(nv) || c->vs_cpu.ensure(nv) ||
            c->vs_mem.ensure(nv) || c->vs_gpu.ensure(nv))
            return FIT_E_OOM;
        HIP_TRY(hipMemcpyAsync(c->vs_off.p, vic_off, bo, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(c->vs_prio.p, vic_prio, b, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(c->vs_cpu.p, vic_cpu, b, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(c->vs_mem.p, vic_mem, b, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(c->vs_gpu.p, vic_gpu, b, hipMemcpyHostToDevice, c->st));
    }
    return load_victims_impl(c, nv > 0 ? vic_off : nullptr, c->vs_off.p, c->vs_prio.p, c->vs_cpu.p, c->vs_mem.p,
                             c->vs_gpu.p);
}

int fit_load_victims_device(fit_ctx* c, const int32_t* vic_off, int64_t n_vic, const int32_t* vic_prio,
                            const int32_t* vic_cpu, const int32_t* vic_mem, const int32_t* vic_gpu) {
    const int rc = check_victims_state(c);
    if (rc) return rc;
    if (n_vic < 0 || n_vic > INT32_MAX || (n_vic > 0 && (!vic_off || !vic_prio || !vic_cpu || !vic_mem || !vic_gpu)))
        return fail(FIT_E_INVAL, "bad victim arrays");
    HIP_TRY(hipSetDevice(c->device));
    if (!vic_off) return load_victims_impl(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    // the lists are judged by a kernel, the offsets come to the host for the row order; the loaded
    // victims stay untouched until the verdict is in
    if (c->vic_bad.ensure(1) || c->h_vic_bad.ensure(1)) return FIT_E_OOM;
    std::vector<int32_t> h_off((size_t)c->n + 1);
    HIP_TRY(hipMemsetAsync(c->vic_bad.p, 0, sizeof(int32_t), c->st));
    HIP_TRY(launch_vic_check(c->st, vic_off, c->n, n_vic, vic_prio, vic_cpu, vic_mem, vic_gpu, c->vic_bad.p));
    HIP_TRY(hipMemcpyAsync(c->h_vic_bad.p, c->vic_bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipMemcpyAsync(h_off.data(), vic_off, sizeof(int32_t) * h_off.size(), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    if (c->h_vic_bad.p[0])
        return fail(FIT_E_INVAL, "victims: vic_off must start at 0, not decrease and end at n_vic; amounts >= 0; "
                                 "priorities non-decreasing inside a node");
    return load_victims_impl(c, n_vic > 0 ? h_off.data() : nullptr, vic_off, vic_prio, vic_cpu, vic_mem, vic_gpu);
}

// fit_preempt / fit_preempt_device: fit_room's tests, then the victims
static int check_preempt_args(fit_ctx* c, int32_t j, std::initializer_list<const void*> arrays) {
    const int rc = check_job_args(c, j, arrays, "fit_preempt", -1);
    if (rc) return rc;
    if (!c->have_vic) return fail(FIT_E_STATE, "fit_load_victims not called");
    return 0;
}

int fit_preempt(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu, const int32_t* wall,
                const uint16_t* part, const int32_t* prio, fit_evict* out) {
    const int rc = check_preempt_args(c, j, {cpu, mem, gpu, wall, part, prio, out});
    if (rc || j == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the priorities ride beside the packed columns: pinned, one copy on the context's stream
    if (c->pe_prio.ensure(j) || c->h_pe_prio.ensure(j)) return FIT_E_OOM;
    memcpy(c->h_pe_prio.p, prio, sizeof(int32_t) * j);
    HIP_TRY(hipMemcpyAsync(c->pe_prio.p, c->h_pe_prio.p, sizeof(int32_t) * j, hipMemcpyHostToDevice, c->st));
    return query_host(
        c, c->pe, j, cpu, mem, gpu, wall, part, nullptr, out,
        [](fit_ctx* x, int32_t n, const JobCols& d, fit_evict* rows, int32_t* bad) {
            return preempt_impl(x, n, d, x->pe_prio.p, rows, bad);
        },
        bad_room_job);
}

int fit_preempt_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                       const int32_t* wall, const uint16_t* part, const int32_t* prio, fit_evict* out) {
    const int rc = check_preempt_args(c, j, {cpu, mem, gpu, wall, part, prio, out});
    if (rc || j == 0) return rc;
    return query_device(
        c, c->pe, j, {cpu, mem, gpu, wall, part, nullptr}, out,
        [&](fit_ctx* x, int32_t n, const JobCols& d, fit_evict* rows, int32_t* bad) {
            return preempt_impl(x, n, d, prio, rows, bad);
        },
        bad_room_job);
}

int fit_preempt_ms(fit_ctx* c, double* ms) {
    if (!c || !ms) return fail(FIT_E_INVAL, "null argument");
    if (c->pe.ms < 0) return fail(FIT_E_STATE, "no fit_preempt_device yet");
    *ms = c->pe.ms;
    return 0;
}

// fit_preempt_k / fit_preempt_k_device: fit_preempt's tests, then kmax (nodes_k against kmax is the
// device's flag word)
static int check_preempt_k_args(fit_ctx* c, int32_t j, std::initializer_list<const void*> arrays, int32_t kmax) {
    const int rc = check_job_args(c, j, arrays, "fit_preempt_k", -1);
    if (rc) return rc;
    if (!c->have_vic) return fail(FIT_E_STATE, "fit_load_victims not called");
    if (kmax < 1 || kmax > FIT_MAX_K) return fail(FIT_E_INVAL, "kmax=%d (1..%d)", kmax, FIT_MAX_K);
    return 0;
}

int fit_preempt_k(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                  const int32_t* wall, const uint16_t* part, const uint16_t* nk, const int32_t* prio, int32_t kmax,
                  fit_evict_k* out, int32_t* out_node, int32_t* out_victims) {
    const int rc = check_preempt_k_args(c, j, {cpu, mem, gpu, wall, part, prio, out, out_node, out_victims}, kmax);
    if (rc || j == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the priorities ride beside the packed columns, as fit_preempt's; the picks come back into pinned
    // memory behind the launches, ahead of query_host's copy of the rows and its synchronisation, and
    // reach the caller only when the call succeeds
    const size_t nn = (size_t)j * kmax;
    if (c->pe_prio.ensure(j) || c->h_pe_prio.ensure(j) || c->pk_node.ensure(nn) || c->pk_vic.ensure(nn) ||
        c->h_pk_pick.ensure(2 * nn))
        return FIT_E_OOM;
    memcpy(c->h_pe_prio.p, prio, sizeof(int32_t) * j);
    HIP_TRY(hipMemcpyAsync(c->pe_prio.p, c->h_pe_prio.p, sizeof(int32_t) * j, hipMemcpyHostToDevice, c->st));
    const int r = query_host(
        c, c->pk, j, cpu, mem, gpu, wall, part, nk, out,
        [&](fit_ctx* x, int32_t n, const JobCols& d, fit_evict_k* rows, int32_t* bad) {
            const int e = preempt_k_impl(x, n, d, x->pe_prio.p, kmax, rows, x->pk_node.p, x->pk_vic.p, bad);
            if (e) return e;
            HIP_TRY(hipMemcpyAsync(x->h_pk_pick.p, x->pk_node.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, x->st));
            HIP_TRY(hipMemcpyAsync(x->h_pk_pick.p + nn, x->pk_vic.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost,
                                   x->st));
            return 0;
        },
        bad_when_k_job);
    if (r) return r;
    memcpy(out_node, c->h_pk_pick.p, sizeof(int32_t) * nn);
    memcpy(out_victims, c->h_pk_pick.p + nn, sizeof(int32_t) * nn);
    return 0;
}

int fit_preempt_k_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                         const int32_t* wall, const uint16_t* part, const uint16_t* nk, const int32_t* prio,
                         int32_t kmax, fit_evict_k* out, int32_t* out_node, int32_t* out_victims) {
    const int rc = check_preempt_k_args(c, j, {cpu, mem, gpu, wall, part, prio, out, out_node, out_victims}, kmax);
    if (rc || j == 0) return rc;
    return query_device(
        c, c->pk, j, {cpu, mem, gpu, wall, part, nk}, out,
        [&](fit_ctx* x, int32_t n, const JobCols& d, fit_evict_k* rows, int32_t* bad) {
            return preempt_k_impl(x, n, d, prio, kmax, rows, out_node, out_victims, bad);
        },
        bad_when_k_job);
}

int fit_preempt_k_ms(fit_ctx* c, double* ms) {
    if (!c || !ms) return fail(FIT_E_INVAL, "null argument");
    if (c->pk.ms < 0) return fail(FIT_E_STATE, "no fit_preempt_k_device yet");
    *ms = c->pk.ms;
    return 0;
}

// fit_load_victims_tl / fit_load_victims_tl_device: fit_load_victims' tests plus the end column
int fit_load_victims_tl(fit_ctx* c, const int32_t* vic_off, const int32_t* vic_prio, const int32_t* vic_end,
                        const int32_t* vic_cpu, const int32_t* vic_mem, const int32_t* vic_gpu) {
    const int rc = check_victims_tl_state(c);
    if (rc) return rc;
    int64_t nv = 0;
    if (vic_off) {  // everything is judged before anything is written: a bad list leaves the loaded lists
        if (vic_off[0] != 0) return fail(FIT_E_INVAL, "vic_off[0] must be 0");
        for (int32_t x = 0; x < c->n; ++x)
            if (vic_off[x + 1] < vic_off[x]) return fail(FIT_E_INVAL, "vic_off decreases at %d", x);
        nv = vic_off[c->n];
        if (nv > 0 && (!vic_prio || !vic_end || !vic_cpu || !vic_mem || !vic_gpu))
            return fail(FIT_E_INVAL, "null victim arrays");
        for (int32_t x = 0; x < c->n; ++x)
            for (int32_t k = vic_off[x]; k < vic_off[x + 1]; ++k) {
                if (vic_cpu[k] < 0 || vic_mem[k] < 0 || vic_gpu[k] < 0)
                    return fail(FIT_E_INVAL, "victim %d of node %d holds a negative amount", k - vic_off[x], x);
                if (vic_end[k] < 0 || vic_end[k] > c->tl_slots)
                    return fail(FIT_E_INVAL, "victim %d of node %d ends at slot %d (0..%d)", k - vic_off[x], x,
                                vic_end[k], c->tl_slots);
                if (k > vic_off[x] && vic_prio[k] < vic_prio[k - 1])
                    return fail(FIT_E_INVAL, "victims of node %d are not in eviction order (priority decreases at %d)",
                                x, k - vic_off[x]);
            }
    }
    HIP_TRY(hipSetDevice(c->device));
    if (nv > 0) {
        const size_t b = sizeof(int32_t) * nv, bo = sizeof(int32_t) * ((size_t)c->n + 1);
        if (c->vs_off.ensure((size_t)c->n + 1) || c->vs_prio.ensure(nv) || c->vs_end.ensure(nv) ||
            c->vs_cpu.ensure(nv) || c->vs_mem.ensure(nv) || c->vs_gpu.ensure(nv))
            return FIT_E_OOM;
        HIP_TRY(hipMemcpyAsync(c->vs_off.p, vic_off, bo, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(c->vs_prio.p, vic_prio, b, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(c->vs_end.p, vic_end, b, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(c->vs_cpu.p, vic_cpu, b, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(c->vs_mem.p, vic_mem, b, hipMemcpyHostToDevice, c->st));
        HIP_TRY(hipMemcpyAsync(c->vs_gpu.p, vic_gpu, b, hipMemcpyHostToDevice, c->st));
    }
    return load_victims_tl_impl(c, nv > 0 ? vic_off : nullptr, c->vs_off.p, c->vs_prio.p, c->vs_end.p, c->vs_cpu.p,
                                c->vs_mem.p, c->vs_gpu.p);
}

int fit_load_victims_tl_device(fit_ctx* c, const int32_t* vic_off, int64_t n_vic, const int32_t* vic_prio,
                               const int32_t* vic_end, const int32_t* vic_cpu, const int32_t* vic_mem,
                               const int32_t* vic_gpu) {
    const int rc = check_victims_tl_state(c);
    if (rc) return rc;
    if (n_vic < 0 || n_vic > INT32_MAX ||
        (n_vic > 0 && (!vic_off || !vic_prio || !vic_end || !vic_cpu || !vic_mem || !vic_gpu)))
        return fail(FIT_E_INVAL, "bad victim arrays");
    HIP_TRY(hipSetDevice(c->device));
    if (!vic_off) return load_victims_tl_impl(c, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
    // judged by a kernel, the offsets come to the host for the position order; the loaded lists stay
    // untouched until the verdict is in
    if (c->vic_bad.ensure(1) || c->h_vic_bad.ensure(1)) return FIT_E_OOM;
    std::vector<int32_t> h_off((size_t)c->n + 1);
    HIP_TRY(hipMemsetAsync(c->vic_bad.p, 0, sizeof(int32_t), c->st));
    HIP_TRY(launch_vtl_check(c->st, vic_off, c->n, n_vic, vic_prio, vic_end, vic_cpu, vic_mem, vic_gpu, c->tl_slots,
                             c->vic_bad.p));
    HIP_TRY(hipMemcpyAsync(c->h_vic_bad.p, c->vic_bad.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipMemcpyAsync(h_off.data(), vic_off, sizeof(int32_t) * h_off.size(), hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    if (c->h_vic_bad.p[0])
        return fail(FIT_E_INVAL, "victims: vic_off must start at 0, not decrease and end at n_vic; amounts >= 0; "
                                 "ends in [0, %d]; priorities non-decreasing inside a node", c->tl_slots);
    return load_victims_tl_impl(c, n_vic > 0 ? h_off.data() : nullptr, vic_off, vic_prio, vic_end, vic_cpu, vic_mem,
                                vic_gpu);
}

// fit_preempt_tl / fit_preempt_tl_device: fit_when's tests, then the timeline's victims
static int check_preempt_tl_args(fit_ctx* c, int32_t j, std::initializer_list<const void*> arrays) {
    const int rc = check_job_args(c, j, arrays, "fit_preempt_tl", 1);
    if (rc) return rc;
    if (!c->have_vtl) return fail(FIT_E_STATE, "fit_load_victims_tl not called");
    return 0;
}

int fit_preempt_tl(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                   const int32_t* wall, const uint16_t* part, const int32_t* prio, fit_evict* out) {
    const int rc = check_preempt_tl_args(c, j, {cpu, mem, gpu, wall, part, prio, out});
    if (rc || j == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the priorities ride beside the packed columns, as fit_preempt's
    if (c->pe_prio.ensure(j) || c->h_pe_prio.ensure(j)) return FIT_E_OOM;
    memcpy(c->h_pe_prio.p, prio, sizeof(int32_t) * j);
    HIP_TRY(hipMemcpyAsync(c->pe_prio.p, c->h_pe_prio.p, sizeof(int32_t) * j, hipMemcpyHostToDevice, c->st));
    return query_host(
        c, c->pt, j, cpu, mem, gpu, wall, part, nullptr, out,
        [](fit_ctx* x, int32_t n, const JobCols& d, fit_evict* rows, int32_t* bad) {
            return preempt_tl_impl(x, n, d, x->pe_prio.p, rows, bad);
        },
        bad_room_job);
}

int fit_preempt_tl_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                          const int32_t* wall, const uint16_t* part, const int32_t* prio, fit_evict* out) {
    const int rc = check_preempt_tl_args(c, j, {cpu, mem, gpu, wall, part, prio, out});
    if (rc || j == 0) return rc;
    return query_device(
        c, c->pt, j, {cpu, mem, gpu, wall, part, nullptr}, out,
        [&](fit_ctx* x, int32_t n, const JobCols& d, fit_evict* rows, int32_t* bad) {
            return preempt_tl_impl(x, n, d, prio, rows, bad);
        },
        bad_room_job);
}

int fit_preempt_tl_ms(fit_ctx* c, double* ms) {
    if (!c || !ms) return fail(FIT_E_INVAL, "null argument");
    if (c->pt.ms < 0) return fail(FIT_E_STATE, "no fit_preempt_tl_device yet");
    *ms = c->pt.ms;
    return 0;
}

// fit_preempt_tl_k / fit_preempt_tl_k_device: fit_preempt_tl's tests, then kmax (nodes_k against kmax is
// the device's flag word)
static int check_preempt_tl_k_args(fit_ctx* c, int32_t j, std::initializer_list<const void*> arrays, int32_t kmax) {
    const int rc = check_job_args(c, j, arrays, "fit_preempt_tl_k", 1);
    if (rc) return rc;
    if (!c->have_vtl) return fail(FIT_E_STATE, "fit_load_victims_tl not called");
    if (kmax < 1 || kmax > FIT_MAX_K) return fail(FIT_E_INVAL, "kmax=%d (1..%d)", kmax, FIT_MAX_K);
    return 0;
}

int fit_preempt_tl_k(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                     const int32_t* wall, const uint16_t* part, const uint16_t* nk, const int32_t* prio, int32_t kmax,
                     fit_evict_k* out, int32_t* out_node, int32_t* out_victims) {
    const int rc = check_preempt_tl_k_args(c, j, {cpu, mem, gpu, wall, part, prio, out, out_node, out_victims}, kmax);
    if (rc || j == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // the priorities and the picks as fit_preempt_k's: staged beside the packed columns, back into
    // pinned memory behind the launches, handed to the caller only when the call succeeds
    const size_t nn = (size_t)j * kmax;
    if (c->pe_prio.ensure(j) || c->h_pe_prio.ensure(j) || c->pk_node.ensure(nn) || c->pk_vic.ensure(nn) ||
        c->h_pk_pick.ensure(2 * nn))
        return FIT_E_OOM;
    memcpy(c->h_pe_prio.p, prio, sizeof(int32_t) * j);
    HIP_TRY(hipMemcpyAsync(c->pe_prio.p, c->h_pe_prio.p, sizeof(int32_t) * j, hipMemcpyHostToDevice, c->st));
    const int r = query_host(
        c, c->ptk, j, cpu, mem, gpu, wall, part, nk, out,
        [&](fit_ctx* x, int32_t n, const JobCols& d, fit_evict_k* rows, int32_t* bad) {
            const int e = preempt_tl_k_impl(x, n, d, x->pe_prio.p, kmax, rows, x->pk_node.p, x->pk_vic.p, bad);
            if (e) return e;
            HIP_TRY(hipMemcpyAsync(x->h_pk_pick.p, x->pk_node.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, x->st));
            HIP_TRY(hipMemcpyAsync(x->h_pk_pick.p + nn, x->pk_vic.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost,
                                   x->st));
            return 0;
        },
        bad_when_k_job);
    if (r) return r;
    memcpy(out_node, c->h_pk_pick.p, sizeof(int32_t) * nn);
    memcpy(out_victims, c->h_pk_pick.p + nn, sizeof(int32_t) * nn);
    return 0;
}

int fit_preempt_tl_k_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                            const int32_t* wall, const uint16_t* part, const uint16_t* nk, const int32_t* prio,
                            int32_t kmax, fit_evict_k* out, int32_t* out_node, int32_t* out_victims) {
    const int rc = check_preempt_tl_k_args(c, j, {cpu, mem, gpu, wall, part, prio, out, out_node, out_victims}, kmax);
    if (rc || j == 0) return rc;
    return query_device(
        c, c->ptk, j, {cpu, mem, gpu, wall, part, nk}, out,
        [&](fit_ctx* x, int32_t n, const JobCols& d, fit_evict_k* rows, int32_t* bad) {
            return preempt_tl_k_impl(x, n, d, prio, kmax, rows, out_node, out_victims, bad);
        },
        bad_when_k_job);
}

int fit_preempt_tl_k_ms(fit_ctx* c, double* ms) {
    if (!c || !ms) return fail(FIT_E_INVAL, "null argument");
    if (c->ptk.ms < 0) return fail(FIT_E_STATE, "no fit_preempt_tl_k_device yet");
    *ms = c->ptk.ms;
    return 0;
}

int fit_read_nodes(fit_ctx* c, int32_t* cpu, int32_t* mem, int32_t* gpu) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (!c->have_nodes) return fail(FIT_E_STATE, "fit_load_nodes not called");
    if (c->n > 0 && (!cpu || !mem || !gpu)) return fail(FIT_E_INVAL, "null output");
    HIP_TRY(hipSetDevice(c->device));
    // scatter into scratch columns seeded with the loaded table: col_* must keep the table of
    // the last fit_load_nodes (fit_load_timeline builds slot 0 from it), whatever was queried
    const size_t b = sizeof(int32_t) * c->n;
    const size_t m = std::max<int32_t>(c->n, 1);
    if (c->rb_cpu.ensure(m) || c->rb_mem.ensure(m) || c->rb_gpu.ensure(m)) return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->rb_cpu.p, c->col_cpu.p, b, hipMemcpyDeviceToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->rb_mem.p, c->col_mem.p, b, hipMemcpyDeviceToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->rb_gpu.p, c->col_gpu.p, b, hipMemcpyDeviceToDevice, c->st));
    HIP_TRY(launch_scatter_nodes(c->st, c->rec.p, c->nn, c->rb_cpu.p, c->rb_mem.p, c->rb_gpu.p));
    HIP_TRY(hipMemcpyAsync(cpu, c->rb_cpu.p, b, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipMemcpyAsync(mem, c->rb_mem.p, b, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipMemcpyAsync(gpu, c->rb_gpu.p, b, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return 0;
}

int fit_partition_free(fit_ctx* c, int32_t p, int64_t* cpu, int64_t* mem, int64_t* gpu) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (p < 0 || p >= 32 || !cpu || !mem || !gpu) return fail(FIT_E_INVAL, "bad partition");
    std::vector<int32_t> hc(c->n), hm(c->n), hg(c->n);
    int rc = fit_read_nodes(c, hc.data(), hm.data(), hg.data());
    if (rc) return rc;
    int64_t sc = 0, sm = 0, sg = 0;
    for (int32_t x = 0; x < c->n; ++x)
        if ((c->h_mask[x] >> p) & 1u) {
            sc += std::max(hc[x], 0);
            sm += std::max(hm[x], 0);
            sg += std::max(hg[x], 0);
        }
    *cpu = sc;
    *mem = sm;
    *gpu = sg;
    return 0;
}

// fit_load_timeline / fit_load_timeline_device: the release events (ne of them; rel_off null: none)
// into rel_*, then the run lists.
static int load_releases(fit_ctx* c, int32_t slots, int32_t slot_min, const int32_t* rel_off, int64_t ne,
                         const int32_t* rel_slot, const int32_t* rel_cpu, const int32_t* rel_mem,
                         const int32_t* rel_gpu, hipMemcpyKind kind) {
    const size_t m = std::max<int64_t>(ne, 1);
    if (c->rel_off.ensure(c->n + 1) || c->rel_slot.ensure(m) || c->rel_cpu.ensure(m) || c->rel_mem.ensure(m) ||
        c->rel_gpu.ensure(m))
        return FIT_E_OOM;
    if (rel_off) {
        HIP_TRY(hipMemcpyAsync(c->rel_off.p, rel_off, sizeof(int32_t) * (c->n + 1), kind, c->st));
        if (ne > 0) {
            const size_t b = sizeof(int32_t) * ne;
            HIP_TRY(hipMemcpyAsync(c->rel_slot.p, rel_slot, b, kind, c->st));
            HIP_TRY(hipMemcpyAsync(c->rel_cpu.p, rel_cpu, b, kind, c->st));
            HIP_TRY(hipMemcpyAsync(c->rel_mem.p, rel_mem, b, kind, c->st));
            HIP_TRY(hipMemcpyAsync(c->rel_gpu.p, rel_gpu, b, kind, c->st));
        }
    }
    return load_timeline_impl(c, slots, slot_min, rel_off ? ne : -1);
}

int fit_load_timeline(fit_ctx* c, int32_t slots, int32_t slot_min, const int32_t* rel_off,
                      const int32_t* rel_slot, const int32_t* rel_cpu, const int32_t* rel_mem,
                      const int32_t* rel_gpu) {
    int rc = check_timeline_args(c, slots, slot_min);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    int64_t ne = 0;
    if (rel_off) {
        if (rel_off[0] != 0) return fail(FIT_E_INVAL, "rel_off[0] must be 0");
        for (int32_t x = 0; x < c->n; ++x)
            if (rel_off[x + 1] < rel_off[x]) return fail(FIT_E_INVAL, "rel_off decreases at %d", x);
        ne = rel_off[c->n];
        if (ne > 0 && (!rel_slot || !rel_cpu || !rel_mem || !rel_gpu))
            return fail(FIT_E_INVAL, "null release arrays");
    }
    return load_releases(c, slots, slot_min, rel_off, ne, rel_slot, rel_cpu, rel_mem, rel_gpu,
                         hipMemcpyHostToDevice);
}

int fit_load_timeline_device(fit_ctx* c, int32_t slots, int32_t slot_min, const int32_t* rel_off,
                             int64_t n_rel, const int32_t* rel_slot, const int32_t* rel_cpu,
                             const int32_t* rel_mem, const int32_t* rel_gpu) {
    int rc = check_timeline_args(c, slots, slot_min);
    if (rc) return rc;
    if (n_rel < 0 || (n_rel > 0 && (!rel_off || !rel_slot || !rel_cpu || !rel_mem || !rel_gpu)))
        return fail(FIT_E_INVAL, "bad release arrays");
    HIP_TRY(hipSetDevice(c->device));
    return load_releases(c, slots, slot_min, rel_off, n_rel, rel_slot, rel_cpu, rel_mem, rel_gpu,
                         hipMemcpyDeviceToDevice);
}

int fit_place_tl(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem,
                 const int32_t* gpu, const int32_t* wall, const uint16_t* part, int32_t* out_node,
                 int32_t* out_start, fit_stats* stats) {
    int rc = check_job_args(c, j, {cpu, mem, gpu, wall, part, out_node, out_start}, nullptr, 1);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    // demands >= 0 are checked on the device (k_prefilter): FIT_E_INVAL
    size_t m = std::max(j, 1);
    JobCols d;
    rc = stage_columns(c, j, cpu, mem, gpu, wall, part, false, nullptr, d);
    if (rc) return rc;
    if (c->out.ensure(m) || c->outs.ensure(m)) return FIT_E_OOM;
    rc = place_tl_impl(c, j, d.cpu, d.mem, d.gpu, d.wall, d.part, c->out.p, c->outs.p, stats);
    if (rc) return rc;
    const size_t b = sizeof(int32_t) * j;
    HIP_TRY(hipMemcpyAsync(out_node, c->out.p, b, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipMemcpyAsync(out_start, c->outs.p, b, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return 0;
}

int fit_place_tl_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem,
                        const int32_t* gpu, const int32_t* wall, const uint16_t* part,
                        int32_t* out_node, int32_t* out_start, fit_stats* stats) {
    int rc = check_job_args(c, j, {cpu, mem, gpu, wall, part, out_node, out_start}, nullptr, 1);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    rc = place_tl_impl(c, j, cpu, mem, gpu, wall, part, out_node, out_start, stats);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->st));
    return 0;
}

// fit_place_tl_k, fit_unplace_tl, fit_hold_tl and their *_device forms: fit_when_k's tests (a query
// name: a sharded context is refused), then kmax; nodes_k against kmax, the demands and the rows
// themselves are the device's flag word
static int check_tl_rows_args(fit_ctx* c, int32_t j, std::initializer_list<const void*> arrays, int32_t kmax,
                              const char* name) {
    const int rc = check_job_args(c, j, arrays, name, 1);
    if (rc) return rc;
    if (kmax < 1 || kmax > FIT_MAX_K) return fail(FIT_E_INVAL, "kmax=%d (1..%d)", kmax, FIT_MAX_K);
    return 0;
}

// the *_ms diagnostic of a timeline writer: value < 0 until its first successful call
static int tl_ms_get(fit_ctx* c, double fit_ctx::*value, const char* name, double* ms) {
    if (!c || !ms) return fail(FIT_E_INVAL, "null argument");
    if (c->*value < 0) return fail(FIT_E_STATE, "no %s yet", name);
    *ms = c->*value;
    return 0;
}

// fit_unplace_tl, fit_hold_tl: the rows from host memory, one copy per column (j > 0)
static int stage_rows(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                      const int32_t* wall, const uint16_t* nk, int32_t kmax, const int32_t* node, const int32_t* start,
                      TlRows& r) {
    const size_t m = j, nn = (size_t)j * kmax, b = sizeof(int32_t) * m;
    if (c->jcpu.ensure(m) || c->jmem.ensure(m) || c->jgpu.ensure(m) || c->jwall.ensure(m) || (nk && c->jk.ensure(m)) ||
        c->tlr_node.ensure(nn) || c->tlr_start.ensure(m))
        return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->jcpu.p, cpu, b, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->jmem.p, mem, b, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->jgpu.p, gpu, b, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->jwall.p, wall, b, hipMemcpyHostToDevice, c->st));
    if (nk) HIP_TRY(hipMemcpyAsync(c->jk.p, nk, sizeof(uint16_t) * m, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->tlr_node.p, node, sizeof(int32_t) * nn, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->tlr_start.p, start, b, hipMemcpyHostToDevice, c->st));
    r = {c->jcpu.p, c->jmem.p, c->jgpu.p, c->jwall.p, nk ? c->jk.p : nullptr, kmax, c->tlr_node.p, c->tlr_start.p};
    return 0;
}

int fit_place_tl_k(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                   const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax, int32_t* out_node,
                   int32_t* out_start, fit_stats* stats) {
    int rc = check_tl_rows_args(c, j, {cpu, mem, gpu, wall, part, out_node, out_start}, kmax, "fit_place_tl_k");
    if (rc) return rc;
    if (j == 0) {
        if (stats) memset(stats, 0, sizeof *stats);
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    JobCols d;
    rc = stage_columns(c, j, cpu, mem, gpu, wall, part, true, nk, d);
    if (rc) return rc;
    const size_t nn = (size_t)j * kmax;
    if (c->out.ensure(nn) || c->outs.ensure(j)) return FIT_E_OOM;
    rc = place_tl_k_impl(c, j, d, kmax, c->out.p, c->outs.p, stats);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out_node, c->out.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipMemcpyAsync(out_start, c->outs.p, sizeof(int32_t) * j, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return 0;
}

int fit_place_tl_k_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                          const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax,
                          int32_t* out_node, int32_t* out_start, fit_stats* stats) {
    const int rc = check_tl_rows_args(c, j, {cpu, mem, gpu, wall, part, out_node, out_start}, kmax, "fit_place_tl_k");
    if (rc) return rc;
    if (j == 0) {
        if (stats) memset(stats, 0, sizeof *stats);
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    return place_tl_k_impl(c, j, {cpu, mem, gpu, wall, part, nk}, kmax, out_node, out_start, stats);
}

int fit_place_tl_k_win(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                       const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax,
                       const int32_t* not_before, const int32_t* deadline, int32_t* out_node, int32_t* out_start,
                       fit_stats* stats) {
    int rc = check_tl_rows_args(c, j, {cpu, mem, gpu, wall, part, out_node, out_start}, kmax, "fit_place_tl_k_win");
    if (rc) return rc;
    if (j == 0) {
        if (stats) memset(stats, 0, sizeof *stats);
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    JobCols d;
    rc = stage_columns(c, j, cpu, mem, gpu, wall, part, true, nk, d);
    if (rc) return rc;
    WinDev w;
    rc = stage_window(c, j, not_before, deadline, w);
    if (rc) return rc;
    const size_t nn = (size_t)j * kmax;
    if (c->out.ensure(nn) || c->outs.ensure(j)) return FIT_E_OOM;
    rc = place_tl_k_impl(c, j, d, kmax, c->out.p, c->outs.p, stats, &w);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out_node, c->out.p, sizeof(int32_t) * nn, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipMemcpyAsync(out_start, c->outs.p, sizeof(int32_t) * j, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return 0;
}

int fit_place_tl_k_win_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                              const int32_t* wall, const uint16_t* part, const uint16_t* nk, int32_t kmax,
                              const int32_t* not_before, const int32_t* deadline, int32_t* out_node,
                              int32_t* out_start, fit_stats* stats) {
    const int rc =
        check_tl_rows_args(c, j, {cpu, mem, gpu, wall, part, out_node, out_start}, kmax, "fit_place_tl_k_win");
    if (rc) return rc;
    if (j == 0) {
        if (stats) memset(stats, 0, sizeof *stats);
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    const WinDev w{not_before, deadline};
    return place_tl_k_impl(c, j, {cpu, mem, gpu, wall, part, nk}, kmax, out_node, out_start, stats, &w);
}

int fit_unplace_tl(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                   const int32_t* wall, const uint16_t* nk, int32_t kmax, const int32_t* node, const int32_t* start,
                   int64_t* applied) {
    int rc = check_tl_rows_args(c, j, {cpu, mem, gpu, wall, node, start}, kmax, "fit_unplace_tl");
    if (rc) return rc;
    if (j == 0) {
        if (applied) *applied = 0;
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    TlRows r;
    rc = stage_rows(c, j, cpu, mem, gpu, wall, nk, kmax, node, start, r);
    return rc ? rc : unplace_tl_impl(c, j, r, applied);
}

int fit_unplace_tl_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                          const int32_t* wall, const uint16_t* nk, int32_t kmax, const int32_t* node,
                          const int32_t* start, int64_t* applied) {
    const int rc = check_tl_rows_args(c, j, {cpu, mem, gpu, wall, node, start}, kmax, "fit_unplace_tl");
    if (rc) return rc;
    if (j == 0) {
        if (applied) *applied = 0;
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    return unplace_tl_impl(c, j, {cpu, mem, gpu, wall, nk, kmax, node, start}, applied);
}

int fit_unplace_tl_ms(fit_ctx* c, double* ms) { return tl_ms_get(c, &fit_ctx::utl_ms, "fit_unplace_tl", ms); }

// fit_evicted_tl / fit_evicted_tl_device, fit_read_victims_tl: fit_preempt_tl's state tests
static int check_evicted_tl_args(fit_ctx* c, int32_t m, std::initializer_list<const void*> arrays, const char* name) {
    const int rc = check_job_args(c, m, arrays, name, 1);
    if (rc) return rc;
    if (!c->have_vtl) return fail(FIT_E_STATE, "fit_load_victims_tl not called");
    return 0;
}

int fit_evicted_tl(fit_ctx* c, int32_t m, const int32_t* node, const int32_t* pos) {
    const int rc = check_evicted_tl_args(c, m, {node, pos}, "fit_evicted_tl");
    if (rc || m == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (c->etl_node.ensure(m) || c->etl_pos.ensure(m)) return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->etl_node.p, node, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->etl_pos.p, pos, sizeof(int32_t) * (size_t)m, hipMemcpyHostToDevice, c->st));
    return evicted_tl_impl(c, m, c->etl_node.p, c->etl_pos.p);
}

int fit_evicted_tl_device(fit_ctx* c, int32_t m, const int32_t* node, const int32_t* pos) {
    const int rc = check_evicted_tl_args(c, m, {node, pos}, "fit_evicted_tl");
    if (rc || m == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return evicted_tl_impl(c, m, node, pos);
}

int fit_evicted_tl_ms(fit_ctx* c, double* ms) { return tl_ms_get(c, &fit_ctx::etl_ms, "fit_evicted_tl", ms); }

// fit_set_tl / fit_set_tl_device: the state tests of fit_unplace_tl; the rows are the device's flag word
int fit_set_tl(fit_ctx* c, int32_t m, const int32_t* node, const int32_t* from, const int32_t* to, const int32_t* cpu,
               const int32_t* mem, const int32_t* gpu, int64_t* applied, int64_t* ignored) {
    const int rc = check_job_args(c, m, {node, from, to, cpu, mem, gpu}, "fit_set_tl", 1);
    if (rc) return rc;
    if (m == 0) {
        if (applied) *applied = 0;
        if (ignored) *ignored = 0;
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    const size_t w = (size_t)m, b = sizeof(int32_t) * w;
    if (c->stl_rows.ensure(6 * w)) return FIT_E_OOM;
    int32_t* d = c->stl_rows.p;
    const int32_t* src[6] = {node, from, to, cpu, mem, gpu};
    for (int i = 0; i < 6; ++i) HIP_TRY(hipMemcpyAsync(d + i * w, src[i], b, hipMemcpyHostToDevice, c->st));
    return set_tl_impl(c, m, d, d + w, d + 2 * w, d + 3 * w, d + 4 * w, d + 5 * w, applied, ignored);
}

int fit_set_tl_device(fit_ctx* c, int32_t m, const int32_t* node, const int32_t* from, const int32_t* to,
                      const int32_t* cpu, const int32_t* mem, const int32_t* gpu, int64_t* applied, int64_t* ignored) {
    const int rc = check_job_args(c, m, {node, from, to, cpu, mem, gpu}, "fit_set_tl", 1);
    if (rc) return rc;
    if (m == 0) {
        if (applied) *applied = 0;
        if (ignored) *ignored = 0;
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    return set_tl_impl(c, m, node, from, to, cpu, mem, gpu, applied, ignored);
}

int fit_set_tl_ms(fit_ctx* c, double* ms) { return tl_ms_get(c, &fit_ctx::stl_ms, "fit_set_tl", ms); }

// The current lists by the caller's node id: the spans and the entries come to the host, which puts
// them in the caller's order (h_perm) and writes every end as the queries read it.
int fit_read_victims_tl(fit_ctx* c, int32_t* off, int64_t cap, int32_t* prio, int32_t* end, int32_t* cpu, int32_t* mem,
                        int32_t* gpu) {
    const int rc = check_evicted_tl_args(c, 0, {}, "fit_read_victims_tl");
    if (rc) return rc;
    if (!off) return fail(FIT_E_INVAL, "null off");
    HIP_TRY(hipSetDevice(c->device));
    std::vector<VicSpan> sp((size_t)std::max(c->nn, 1));
    std::vector<VicTl> ent((size_t)std::max(c->vtl_total, 1));
    HIP_TRY(hipMemcpyAsync(sp.data(), c->vtl_span.p, sizeof(VicSpan) * sp.size(), hipMemcpyDeviceToHost, c->st));
    if (c->vtl_total > 0)
        HIP_TRY(hipMemcpyAsync(ent.data(), c->vtl_ent.p, sizeof(VicTl) * (size_t)c->vtl_total, hipMemcpyDeviceToHost,
                               c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    for (int32_t x = 0; x <= c->n; ++x) off[x] = 0;
    for (int32_t i = 0; i < c->nn; ++i) off[c->h_perm[i] + 1] = sp[i].len;  // a node in no partition: empty
    for (int32_t x = 0; x < c->n; ++x) off[x + 1] += off[x];
    if (!prio || !end || !cpu || !mem || !gpu || cap < off[c->n]) return 0;
    for (int32_t i = 0; i < c->nn; ++i) {
        const VicTl* e = ent.data() + sp[i].beg;
        for (int32_t k = 0, d = off[c->h_perm[i]]; k < sp[i].len; ++k, ++d) {
            prio[d] = e[k].prio;
            end[d] = std::max(e[k].end - c->vtl_shift, 0);
            cpu[d] = e[k].cpu;
            mem[d] = e[k].mem;
            gpu[d] = e[k].gpu;
        }
    }
    return 0;
}

// fit_hold_tl: out_state among the arrays
int fit_hold_tl(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                const int32_t* wall, const uint16_t* nk, int32_t kmax, const int32_t* node, const int32_t* start,
                int32_t* out_state, int64_t* applied, int64_t* refused) {
    int rc = check_tl_rows_args(c, j, {cpu, mem, gpu, wall, node, start, out_state}, kmax, "fit_hold_tl");
    if (rc) return rc;
    if (j == 0) {
        if (applied) *applied = 0;
        if (refused) *refused = 0;
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    TlRows r;
    rc = stage_rows(c, j, cpu, mem, gpu, wall, nk, kmax, node, start, r);
    if (rc) return rc;
    if (c->tlr_state.ensure(j)) return FIT_E_OOM;
    rc = hold_tl_impl(c, j, r, c->tlr_state.p, applied, refused);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out_state, c->tlr_state.p, sizeof(int32_t) * (size_t)j, hipMemcpyDeviceToHost, c->st));
    HIP_TRY(hipStreamSynchronize(c->st));
    return 0;
}

int fit_hold_tl_device(fit_ctx* c, int32_t j, const int32_t* cpu, const int32_t* mem, const int32_t* gpu,
                       const int32_t* wall, const uint16_t* nk, int32_t kmax, const int32_t* node,
                       const int32_t* start, int32_t* out_state, int64_t* applied, int64_t* refused) {
    const int rc = check_tl_rows_args(c, j, {cpu, mem, gpu, wall, node, start, out_state}, kmax, "fit_hold_tl");
    if (rc) return rc;
    if (j == 0) {
        if (applied) *applied = 0;
        if (refused) *refused = 0;
        return 0;
    }
    HIP_TRY(hipSetDevice(c->device));
    return hold_tl_impl(c, j, {cpu, mem, gpu, wall, nk, kmax, node, start}, out_state, applied, refused);
}

int fit_hold_tl_ms(fit_ctx* c, double* ms) { return tl_ms_get(c, &fit_ctx::htl_ms, "fit_hold_tl", ms); }

// fit_advance_tl / fit_advance_tl_device: the state tests of fit_unplace_tl, then a and the pointers
static int check_advance_tl_args(fit_ctx* c, int32_t a, const int32_t* tc, const int32_t* tm, const int32_t* tg) {
    const int rc = check_job_args(c, 0, {}, "fit_advance_tl", 1);
    if (rc) return rc;
    if (a < 0) return fail(FIT_E_INVAL, "a=%d", a);
    if (a > 0 && ((!tc != !tm) || (!tc != !tg))) return fail(FIT_E_INVAL, "some but not all tail pointers are NULL");
    return 0;
}

int fit_advance_tl(fit_ctx* c, int32_t a, const int32_t* tc, const int32_t* tm, const int32_t* tg) {
    const int rc = check_advance_tl_args(c, a, tc, tm, tg);
    if (rc || a == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    if (!tc || c->n == 0) return advance_tl_impl(c, a, nullptr, nullptr, nullptr);
    const size_t m = c->n, b = sizeof(int32_t) * m;
    if (c->atl_tc.ensure(m) || c->atl_tm.ensure(m) || c->atl_tg.ensure(m)) return FIT_E_OOM;
    HIP_TRY(hipMemcpyAsync(c->atl_tc.p, tc, b, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->atl_tm.p, tm, b, hipMemcpyHostToDevice, c->st));
    HIP_TRY(hipMemcpyAsync(c->atl_tg.p, tg, b, hipMemcpyHostToDevice, c->st));
    return advance_tl_impl(c, a, c->atl_tc.p, c->atl_tm.p, c->atl_tg.p);
}

int fit_advance_tl_device(fit_ctx* c, int32_t a, const int32_t* tc, const int32_t* tm, const int32_t* tg) {
    const int rc = check_advance_tl_args(c, a, tc, tm, tg);
    if (rc || a == 0) return rc;
    HIP_TRY(hipSetDevice(c->device));
    return advance_tl_impl(c, a, tc, tm, tg);
}

int fit_advance_tl_ms(fit_ctx* c, double* ms) { return tl_ms_get(c, &fit_ctx::atl_ms, "fit_advance_tl", ms); }

// fit_free_tl / fit_free_tl_device: read-only, so a HIP error fails the call
// and the timeline stays loaded.  rows: device, parts * H of them, valid when the stream has drained.
static int free_tl_impl(fit_ctx* c, int32_t parts, fit_free* rows) {
    static_assert(sizeof(fit_free) == FREE_ROW_BYTES, "fit_free is 40 bytes");
    const size_t n = (size_t)parts * c->tl_slots;
    if (c->free_acc.ensure(n * (FREE_ROW_BYTES / sizeof(int64_t)))) return FIT_E_OOM;
    int32_t chunk = FREE_CHUNK;  // FIT_FREE_CHUNK: measurements (tools/free_tl_bench.py)
    if (const char* e = getenv("FIT_FREE_CHUNK")) chunk = std::max(1, std::min(atoi(e), FREE_MAX_CHUNK));
    HIP_TRY(hipEventRecord(c->ev[0], c->st));
    HIP_TRY(launch_free_tl(c->st, c->tlhdr.p, c->slab.p, c->nn, c->tl_slots, parts, chunk, c->free_acc.p, rows));
    HIP_TRY(hipEventRecord(c->ev[1], c->st));
    return 0;
}
static int free_tl_done(fit_ctx* c) {
    float ms = 0.f;
    HIP_TRY(hipStreamSynchronize(c->st));
    HIP_TRY(hipEventElapsedTime(&ms, c->ev[0], c->ev[1]));
    c->free_ms = ms;
    return 0;
}
static int check_free_tl_args(fit_ctx* c, int32_t parts, const fit_free* out) {
    if (!c || !out) return fail(FIT_E_INVAL, "null argument");
    if (parts < 1 || parts > 32) return fail(FIT_E_INVAL, "parts=%d (1..32)", parts);
    return check_job_args(c, 0, {}, "fit_free_tl", 1);
}

int fit_free_tl(fit_ctx* c, int32_t parts, fit_free* out) {
    int rc = check_free_tl_args(c, parts, out);
    if (rc) return rc;
    HIP_TRY(hipSetDevice(c->device));
    const size_t n = (size_t)parts * c->tl_slots;
    if (c->free_rows.ensure(n)) return FIT_E_OOM;
    rc = free_tl_impl(c, parts, c->free_rows.p);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(out, c->free_rows.p, sizeof(fit_free) * n, hipMemcpyDeviceToHost, c->st));
    return free_tl_done(c);
}

int fit_free_tl_device(fit_ctx* c, int32_t parts, fit_free* out) {
    int rc = check_free_tl_args(c, parts, out);
    if (rc) return rc;
    if ((uintptr_t)out & 7u) return fail(FIT_E_INVAL, "out is not 8-byte aligned");
    HIP_TRY(hipSetDevice(c->device));
    rc = free_tl_impl(c, parts, out);
    return rc ? rc : free_tl_done(c);
}

int fit_free_tl_ms(fit_ctx* c, double* ms) { return tl_ms_get(c, &fit_ctx::free_ms, "fit_free_tl", ms); }

int fit_read_timeline(fit_ctx* c, int32_t* cpu, int32_t* mem, int32_t* gpu) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (!c->have_tl) return fail(FIT_E_STATE, "fit_load_timeline not called");
    if (c->n > 0 && (!cpu || !mem || !gpu)) return fail(FIT_E_INVAL, "null output");
    HIP_TRY(hipSetDevice(c->device));
    const size_t cells = (size_t)c->n * c->tl_slots;
    DBuf<int32_t> d[3];
    for (auto& x : d)
        if (x.ensure(std::max<size_t>(cells, 1))) return FIT_E_OOM;
    // rows of nodes outside every partition (mask 0) are not on the device: -1, like unusable
    int rc = 0;
    for (auto& x : d)
        if (hipMemsetAsync(x.p, 0xff, sizeof(int32_t) * cells, c->st) != hipSuccess) rc = FIT_E_HIP;
    if (rc || launch_expand_tl(c->st, c->perm.p, c->slab.p, c->tlhdr.p, c->nn, c->tl_slots, d[0].p,
                         d[1].p, d[2].p) != hipSuccess ||
        hipMemcpyAsync(cpu, d[0].p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
        hipMemcpyAsync(mem, d[1].p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
        hipMemcpyAsync(gpu, d[2].p, sizeof(int32_t) * cells, hipMemcpyDeviceToHost, c->st) != hipSuccess ||
        hipStreamSynchronize(c->st) != hipSuccess)
        rc = fail(FIT_E_HIP, "timeline read-back failed");
    return rc;
}

}  // extern "C"

namespace fitgpu {
void set_last_error(const char* msg) { g_last_error = msg; }  // admit.cpp: the batch's error

// admit.cpp: the context's table as the admitter's host copy starts from it (a table loaded with
// fit_load_nodes directly, before the admitter manages it).  Free columns as fit_read_nodes
// gives them (current, after placements); avail / mask as loaded.
int64_t ctx_load_count(const fit_ctx* c) { return c && c->have_nodes ? c->loads : 0; }
int ctx_table(fit_ctx* c, std::vector<int32_t>& cpu, std::vector<int32_t>& mem,
              std::vector<int32_t>& gpu, std::vector<int32_t>& avail, std::vector<uint32_t>& mask) {
    if (!c) return fail(FIT_E_INVAL, "null ctx");
    if (!c->have_nodes) return fail(FIT_E_STATE, "no node table loaded");
    const size_t m = std::max<int32_t>(c->n, 1);
    cpu.resize(m), mem.resize(m), gpu.resize(m), avail.resize(m);
    const int rc = fit_read_nodes(c, cpu.data(), mem.data(), gpu.data());
    if (rc) return rc;
    HIP_TRY(hipMemcpy(avail.data(), c->col_av.p, sizeof(int32_t) * c->n, hipMemcpyDeviceToHost));
    cpu.resize(c->n), mem.resize(c->n), gpu.resize(c->n), avail.resize(c->n);
    mask = c->h_mask;
    return 0;
}
}  // namespace fitgpu

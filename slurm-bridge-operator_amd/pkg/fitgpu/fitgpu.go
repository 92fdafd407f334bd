// Package fitgpu is the cgo binding a slurm-bridge-operator maintainer adds to call the MI355X
// placement engine (libfitgpu.so, C-ABI include/fitgpu.h).  It is not compiled in this repo's
// image (no Go toolchain); INTEGRATION.md shows where it is called from.
package fitgpu

/*
#cgo CFLAGS: -I${SRCDIR}/../../../include
#cgo LDFLAGS: -L${SRCDIR}/../../fitgpu -lfitgpu -Wl,-rpath,${SRCDIR}/../../fitgpu
#include <stdlib.h>
#include "fitgpu.h"
*/
import "C"

import (
	"errors"
	"fmt"
	"runtime"
	"unsafe"
)

const (
	Unplaced = -1 // FIT_UNPLACED
	Rejected = -2 // FIT_REJECTED
	MaxK     = 8  // FIT_MAX_K: nodes per job (--nodes) fit_place supports
)

// Error carries a negative FIT_E_* code and the library's detail message.
type Error struct {
	Code   int
	Detail string
}

func (e *Error) Error() string {
	return fmt.Sprintf("fitgpu: %s (%d): %s", C.GoString(C.fit_strerror(C.int(e.Code))), e.Code, e.Detail)
}

// EngineFailure reports whether err is the engine failing rather than a decision about a pod:
// a HIP / RCCL runtime error (a watchdog trip included), an allocation failure, no device, or
// a context out of state.  Callers fall back to the reference path on these (INTEGRATION.md).
func EngineFailure(err error) bool {
	var fe *Error
	if !errors.As(err, &fe) {
		return false
	}
	switch fe.Code {
	case int(C.FIT_E_HIP), int(C.FIT_E_RCCL), int(C.FIT_E_OOM), int(C.FIT_E_NODEV), int(C.FIT_E_STATE):
		return true
	}
	return false
}

// SetWatchdog bounds every device-side wait of the persistent engines (fit_set_watchdog_us);
// us <= 0 restores the default (10 s).
func (e *Engine) SetWatchdog(us int64) error {
	return check(C.fit_set_watchdog_us(e.ctx, C.int64_t(us)))
}

// LockDir is the directory of the per-GPU lock file that serialises persistent launches of
// every engine on a GPU (fit_lock_dir).  shared is false when the library fell back to /tmp: in
// the configurator's deployment each virtual kubelet is its own pod with a private /tmp, so
// engines in other pods on the same GPU would not be arbitrated (INTEGRATION.md item 6).
func LockDir() (dir string, shared bool, err error) {
	buf := make([]byte, 4096)
	rc := C.fit_lock_dir((*C.char)(unsafe.Pointer(&buf[0])), C.int32_t(len(buf)))
	if err := check(rc); err != nil {
		return "", false, err
	}
	return C.GoString((*C.char)(unsafe.Pointer(&buf[0]))), rc == 0, nil
}

func check(rc C.int) error {
	if rc < 0 {
		return &Error{Code: int(rc), Detail: C.GoString(C.fit_last_error())}
	}
	return nil
}

// Engine wraps one fit_ctx (one GPU).  Not safe for concurrent use; the VK provider serialises
// its 10 PodSyncWorkers through a batcher (INTEGRATION.md).
type Engine struct {
	ctx   *C.fit_ctx
	slots int // horizon of the last successful LoadTimeline (FreeTL sizes its rows by it)
	nodes int // rows of the last successful LoadNodes (ReadVictimsTL sizes Off by it)
}

func New(device int) (*Engine, error) {
	opts := C.fit_opts{device: C.int32_t(device), world: 1}
	var ctx *C.fit_ctx
	if err := check(C.fit_create(&opts, &ctx)); err != nil {
		return nil, err
	}
	e := &Engine{ctx: ctx}
	runtime.SetFinalizer(e, func(e *Engine) { e.Close() })
	return e, nil
}

func (e *Engine) Close() {
	if e.ctx != nil {
		C.fit_destroy(e.ctx)
		e.ctx = nil
	}
}

// Nodes is the node table in Client.Nodes order (pkg/slurm-agent/slurm.go:343-364).
type Nodes struct {
	CPUFree, MemFreeMiB, GPUFree, AvailMin []int32
	PartMask                              []uint32
}

// errLen is returned when the columns of one table differ in length: the library reads every
// column for the same count, so a short slice would be read past its end.
var errLen = errors.New("fitgpu: column slices of different lengths")

func sameLen(n int, cols ...int) bool {
	for _, c := range cols {
		if c != n {
			return false
		}
	}
	return true
}

func (e *Engine) LoadNodes(n Nodes) error {
	cnt := len(n.CPUFree)
	if !sameLen(cnt, len(n.MemFreeMiB), len(n.GPUFree), len(n.AvailMin), len(n.PartMask)) {
		return errLen
	}
	if cnt == 0 {
		err := check(C.fit_load_nodes(e.ctx, 0, nil, nil, nil, nil, nil))
		if err == nil {
			e.nodes = 0
		}
		return err
	}
	// slices of plain integers: no Go pointers inside, the library copies and does not retain
	rc := C.fit_load_nodes(e.ctx, C.int32_t(cnt),
		(*C.int32_t)(unsafe.Pointer(&n.CPUFree[0])), (*C.int32_t)(unsafe.Pointer(&n.MemFreeMiB[0])),
		(*C.int32_t)(unsafe.Pointer(&n.GPUFree[0])), (*C.int32_t)(unsafe.Pointer(&n.AvailMin[0])),
		(*C.uint32_t)(unsafe.Pointer(&n.PartMask[0])))
	runtime.KeepAlive(e) // the finalizer must not destroy the context during the call
	err := check(rc)
	if err == nil {
		e.nodes = cnt
	}
	return err
}

// LoadPartitions takes parseResources' limits (pkg/slurm-agent/parse.go:111-190), -1 = UNLIMITED.
func (e *Engine) LoadPartitions(maxTimeMin, maxCPUs, maxMemMiB []int32) error {
	p := len(maxTimeMin)
	if !sameLen(p, len(maxCPUs), len(maxMemMiB)) {
		return errLen
	}
	if p == 0 {
		return check(C.fit_load_partitions(e.ctx, 0, nil, nil, nil))
	}
	return check(C.fit_load_partitions(e.ctx, C.int32_t(p), (*C.int32_t)(unsafe.Pointer(&maxTimeMin[0])),
		(*C.int32_t)(unsafe.Pointer(&maxCPUs[0])), (*C.int32_t)(unsafe.Pointer(&maxMemMiB[0]))))
}

// Jobs in priority order, per-node demand (DESIGN.md §2).
type Jobs struct {
	CPU, MemMiB, GPU, WallMin []int32
	Part, NodesK              []uint16
}

type Stats = C.fit_stats

// Place returns node ids (or Unplaced / Rejected) per job, kmax entries per job.
// NodesK may be empty (every job takes one node); otherwise it has one entry per job.
func (e *Engine) Place(j Jobs, kmax int) ([]int32, Stats, error) {
	cnt := len(j.CPU)
	var st C.fit_stats
	if kmax < 1 || kmax > MaxK {
		return nil, st, fmt.Errorf("fitgpu: kmax %d outside [1, %d]", kmax, MaxK)
	}
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part)) ||
		(len(j.NodesK) != 0 && len(j.NodesK) != cnt) {
		return nil, st, errLen
	}
	out := make([]int32, cnt*kmax)
	if cnt == 0 {
		return out, st, nil
	}
	var nk *C.uint16_t // NULL: every job takes one node
	if len(j.NodesK) > 0 {
		nk = (*C.uint16_t)(unsafe.Pointer(&j.NodesK[0]))
	}
	rc := C.fit_place(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])),
		nk, C.int32_t(kmax), (*C.int32_t)(unsafe.Pointer(&out[0])), &st)
	runtime.KeepAlive(e)
	return out, st, check(rc)
}

// Why codes (fit_why.code, include/fitgpu.h): why a job does not fit, or that it does.
const (
	WhyFits      = int32(C.FIT_WHY_FITS)
	WhyPartition = int32(C.FIT_WHY_PARTITION)
	WhyLimitTime = int32(C.FIT_WHY_LIMIT_TIME)
	WhyLimitCPUs = int32(C.FIT_WHY_LIMIT_CPUS)
	WhyLimitMem  = int32(C.FIT_WHY_LIMIT_MEM)
	WhyNoNodes   = int32(C.FIT_WHY_NO_NODES)
	WhyResources = int32(C.FIT_WHY_RESOURCES)
)

// Why is one fit_why row: the job judged alone against the current node table.  The Short*
// counts overlap, as kube-scheduler's do (a node short of two things is counted twice).
type Why struct {
	Code      int32 // Why*
	Need      int32 // nodes the job needs (--nodes, at least 1)
	Members   int32 // schedulable nodes of the job's partition
	Fit       int32 // members the job fits on now
	ShortCPU  int32
	ShortMem  int32
	ShortGPU  int32
	ShortTime int32
}

func goWhy(w *C.fit_why) Why {
	return Why{Code: int32(w.code), Need: int32(w.need), Members: int32(w.members), Fit: int32(w.fit),
		ShortCPU: int32(w.short_cpu), ShortMem: int32(w.short_mem), ShortGPU: int32(w.short_gpu),
		ShortTime: int32(w.short_time)}
}

// Explain diagnoses every job alone against the current node table (fit_explain); it changes
// nothing.  NodesK may be empty, as for Place.
func (e *Engine) Explain(j Jobs) ([]Why, error) {
	cnt := len(j.CPU)
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part)) ||
		(len(j.NodesK) != 0 && len(j.NodesK) != cnt) {
		return nil, errLen
	}
	if cnt == 0 {
		return nil, nil
	}
	var nk *C.uint16_t
	if len(j.NodesK) > 0 {
		nk = (*C.uint16_t)(unsafe.Pointer(&j.NodesK[0]))
	}
	rows := make([]C.fit_why, cnt)
	rc := C.fit_explain(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])), nk, &rows[0])
	runtime.KeepAlive(e)
	if err := check(rc); err != nil {
		return nil, err
	}
	out := make([]Why, cnt)
	for i := range rows {
		out[i] = goWhy(&rows[i])
	}
	return out, nil
}

// PartitionFree is the allocation-aware replacement for GetPartitionCapacity's sum
// (pkg/slurm-virtual-kubelet/node.go:183-190).
func (e *Engine) PartitionFree(p int) (cpu, memMiB, gpu int64, err error) {
	var c, m, g C.int64_t
	err = check(C.fit_partition_free(e.ctx, C.int32_t(p), &c, &m, &g))
	runtime.KeepAlive(e)
	return int64(c), int64(m), int64(g), err
}

// Releases are the end times of the jobs already running on each node (squeue EndTime), CSR by
// node id: node x's events are [Off[x], Off[x+1]) with non-decreasing Slot (DESIGN.md §2b).
type Releases struct {
	Off, Slot, CPU, MemMiB, GPU []int32
}

// LoadTimeline builds the backfill horizon (slots of slotMin minutes, <= 1024 slots) on top of
// the node table of the last LoadNodes.
func (e *Engine) LoadTimeline(slots, slotMin int, r Releases) error {
	if !sameLen(len(r.Slot), len(r.CPU), len(r.MemMiB), len(r.GPU)) {
		return errLen
	}
	if len(r.Off) > 0 && int(r.Off[len(r.Off)-1]) > len(r.Slot) {
		return fmt.Errorf("fitgpu: Off ends at %d but there are %d release events", r.Off[len(r.Off)-1], len(r.Slot))
	}
	var err error
	if len(r.Off) == 0 {
		err = check(C.fit_load_timeline(e.ctx, C.int32_t(slots), C.int32_t(slotMin), nil, nil, nil, nil, nil))
	} else {
		var s, c, m, g *C.int32_t
		if len(r.Slot) > 0 {
			s, c = (*C.int32_t)(unsafe.Pointer(&r.Slot[0])), (*C.int32_t)(unsafe.Pointer(&r.CPU[0]))
			m, g = (*C.int32_t)(unsafe.Pointer(&r.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&r.GPU[0]))
		}
		err = check(C.fit_load_timeline(e.ctx, C.int32_t(slots), C.int32_t(slotMin),
			(*C.int32_t)(unsafe.Pointer(&r.Off[0])), s, c, m, g))
	}
	if err == nil {
		e.slots = slots
	}
	return err
}

// RunningJob is one job the caller knows is running (the virtual kubelet's own pods): its engine
// node rows (JobInfo.node_list expanded with ExpandHostlist, mapped through the NodeNames table),
// the minutes left until JobInfo.end_time (workload.proto:252-292) and its per-node demand.
type RunningJob struct {
	Nodes            []int32
	MinutesLeft      int64
	CPU, MemMiB, GPU int32
}

// ReleaseEvents turns running jobs into the release events LoadTimeline reads
// (fit_release_events): each job hands its demand back on each of its nodes at slot
// max(1, ceil(MinutesLeft / slotMin)), capped at the horizon.
func ReleaseEvents(nodes int, jobs []RunningJob, slots, slotMin int) (Releases, error) {
	off := make([]int32, len(jobs)+1)
	var rows []int32
	rem := make([]int64, len(jobs))
	cpu, mem, gpu := make([]int32, len(jobs)), make([]int32, len(jobs)), make([]int32, len(jobs))
	for i, j := range jobs {
		rows = append(rows, j.Nodes...)
		off[i+1] = int32(len(rows))
		rem[i], cpu[i], mem[i], gpu[i] = j.MinutesLeft, j.CPU, j.MemMiB, j.GPU
	}
	e := len(rows)
	r := Releases{Off: make([]int32, nodes+1), Slot: make([]int32, e), CPU: make([]int32, e),
		MemMiB: make([]int32, e), GPU: make([]int32, e)}
	p32 := func(v []int32) *C.int32_t {
		if len(v) == 0 {
			return nil
		}
		return (*C.int32_t)(unsafe.Pointer(&v[0]))
	}
	var remp *C.int64_t
	if len(rem) > 0 {
		remp = (*C.int64_t)(unsafe.Pointer(&rem[0]))
	}
	n := C.fit_release_events(C.int32_t(nodes), C.int32_t(len(jobs)), p32(off), p32(rows), remp, p32(cpu),
		p32(mem), p32(gpu), C.int32_t(slots), C.int32_t(slotMin), p32(r.Off), p32(r.Slot), p32(r.CPU),
		p32(r.MemMiB), p32(r.GPU), C.int32_t(e))
	runtime.KeepAlive(rows)
	if err := check(n); err != nil {
		return Releases{}, err
	}
	return r, nil
}

// PlaceBackfill gives each job (one node) its node and earliest start slot (DESIGN.md §2b);
// node is Unplaced when nothing fits inside the horizon, Rejected for partition limits.
func (e *Engine) PlaceBackfill(j Jobs) (node, start []int32, st Stats, err error) {
	cnt := len(j.CPU)
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part)) {
		return nil, nil, st, errLen
	}
	node, start = make([]int32, cnt), make([]int32, cnt)
	if cnt == 0 {
		return node, start, st, nil
	}
	rc := C.fit_place_tl(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])),
		(*C.int32_t)(unsafe.Pointer(&node[0])), (*C.int32_t)(unsafe.Pointer(&start[0])), &st)
	runtime.KeepAlive(e)
	return node, start, st, check(rc)
}

// PlaceTLK is PlaceBackfill for jobs of NodesK nodes (DESIGN.md §2g): the queue in index order, each
// job reserved on all of its nodes from one common start, against the timeline as the jobs before it
// left it.  nodes has kmax entries per job: a placed job's nodes in key order, -1 elsewhere;
// nodes[q*kmax] is Rejected for partition limits, and Unplaced (like the rest) when no start has
// NodesK nodes free together inside the horizon.  start[q] is the start slot, -1 when not placed.
// NodesK may be empty (every job takes one node); otherwise it has one entry per job.
func (e *Engine) PlaceTLK(j Jobs, kmax int) (nodes, start []int32, st Stats, err error) {
	cnt := len(j.CPU)
	if kmax < 1 || kmax > MaxK {
		return nil, nil, st, fmt.Errorf("fitgpu: kmax %d outside [1, %d]", kmax, MaxK)
	}
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part)) ||
		(len(j.NodesK) != 0 && len(j.NodesK) != cnt) {
		return nil, nil, st, errLen
	}
	nodes, start = make([]int32, cnt*kmax), make([]int32, cnt)
	if cnt == 0 {
		return nodes, start, st, nil
	}
	var nk *C.uint16_t // NULL: every job takes one node
	if len(j.NodesK) > 0 {
		nk = (*C.uint16_t)(unsafe.Pointer(&j.NodesK[0]))
	}
	rc := C.fit_place_tl_k(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])),
		nk, C.int32_t(kmax), (*C.int32_t)(unsafe.Pointer(&nodes[0])), (*C.int32_t)(unsafe.Pointer(&start[0])), &st)
	runtime.KeepAlive(e)
	return nodes, start, st, check(rc)
}

// winCols gives the two optional window columns of PlaceTLKWin as C pointers: an empty
// slice is NULL (notBefore: all 0, deadline: none), any other has one entry per job.
func winCols(cnt int, notBefore, deadline []int32) (nb, dl *C.int32_t, err error) {
	if (len(notBefore) != 0 && len(notBefore) != cnt) || (len(deadline) != 0 && len(deadline) != cnt) {
		return nil, nil, errLen
	}
	if len(notBefore) > 0 {
		nb = (*C.int32_t)(unsafe.Pointer(&notBefore[0]))
	}
	if len(deadline) > 0 {
		dl = (*C.int32_t)(unsafe.Pointer(&deadline[0]))
	}
	return nb, dl, nil
}

// PlaceTLKWin is PlaceTLK with a window of allowed starts per job (DESIGN.md §2r): job q may start
// at slot s only when clamp(notBefore[q], 0, H) <= s and s + d <= clamp(deadline[q], 0, H), d =
// max(1, ceil(WallMin/slotMin)) — `sbatch --begin` / `--deadline` in slots, the planned end
// start + d of a dependency's parent, the recorded start of a row HoldTL refused.  No value is an
// error: a negative notBefore is 0, a deadline <= 0 has passed, math.MaxInt32 is none.  A job
// without an allowed start is Unplaced and consumes nothing.  Empty notBefore / deadline: all 0 /
// none; with both empty the result is PlaceTLK's.  Outputs and st as PlaceTLK.
func (e *Engine) PlaceTLKWin(j Jobs, kmax int, notBefore, deadline []int32) (nodes, start []int32, st Stats, err error) {
	cnt := len(j.CPU)
	if kmax < 1 || kmax > MaxK {
		return nil, nil, st, fmt.Errorf("fitgpu: kmax %d outside [1, %d]", kmax, MaxK)
	}
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part)) ||
		(len(j.NodesK) != 0 && len(j.NodesK) != cnt) {
		return nil, nil, st, errLen
	}
	nb, dl, err := winCols(cnt, notBefore, deadline)
	if err != nil {
		return nil, nil, st, err
	}
	nodes, start = make([]int32, cnt*kmax), make([]int32, cnt)
	if cnt == 0 {
		return nodes, start, st, nil
	}
	var nk *C.uint16_t // NULL: every job takes one node
	if len(j.NodesK) > 0 {
		nk = (*C.uint16_t)(unsafe.Pointer(&j.NodesK[0]))
	}
	rc := C.fit_place_tl_k_win(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])),
		nk, C.int32_t(kmax), nb, dl, (*C.int32_t)(unsafe.Pointer(&nodes[0])),
		(*C.int32_t)(unsafe.Pointer(&start[0])), &st)
	runtime.KeepAlive(e)
	return nodes, start, st, check(rc)
}

// UnplaceTL hands reservations back to the loaded timeline (DESIGN.md §2h): row q adds its per-node
// demand to slots [start[q], start[q]+d) of node[q*kmax .. +max(NodesK,1)), d = max(1,
// ceil(WallMin/slotMin)).  j, node and start are the columns given to, and returned by, PlaceTLK
// (kmax 1: PlaceBackfill); rows with start[q] < 0 are skipped, so a placement's outputs go back
// verbatim.  j.Part is not used.  A job seen to end early is unplaced with start 0 and its
// remaining minutes as WallMin.  Returns the (row, node) windows added.
func (e *Engine) UnplaceTL(j Jobs, kmax int, node, start []int32) (int64, error) {
	cnt := len(j.CPU)
	if kmax < 1 || kmax > MaxK {
		return 0, fmt.Errorf("fitgpu: kmax %d outside [1, %d]", kmax, MaxK)
	}
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(start)) || len(node) != cnt*kmax ||
		(len(j.NodesK) != 0 && len(j.NodesK) != cnt) {
		return 0, errLen
	}
	if cnt == 0 {
		return 0, nil
	}
	var nk *C.uint16_t // NULL: every job took one node
	if len(j.NodesK) > 0 {
		nk = (*C.uint16_t)(unsafe.Pointer(&j.NodesK[0]))
	}
	var applied C.int64_t
	rc := C.fit_unplace_tl(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), nk, C.int32_t(kmax),
		(*C.int32_t)(unsafe.Pointer(&node[0])), (*C.int32_t)(unsafe.Pointer(&start[0])), &applied)
	runtime.KeepAlive(e)
	return int64(applied), check(rc)
}

// Hold states (out_state of fit_hold_tl, include/fitgpu.h).
const (
	HoldHeld    = int32(C.FIT_HOLD_HELD)
	HoldRefused = int32(C.FIT_HOLD_REFUSED)
	HoldSkipped = int32(C.FIT_HOLD_SKIPPED)
)

// HoldTL re-applies recorded reservations to the loaded timeline (DESIGN.md §2j), after a reload,
// a dropped timeline or a restart: row q subtracts its per-node demand from slots [start[q],
// start[q]+d) of node[q*kmax .. +max(NodesK,1)) — the recorded nodes and start, nothing is chosen
// again — unless on one of those slots the demands of all live rows of the call together exceed
// what the timeline holds; then every row that covers the slot is refused and nothing of it is
// subtracted.  j, node and start are UnplaceTL's; rows with start[q] < 0 are skipped.  j.Part is not
// used.  Returns the state of every row (HoldHeld, HoldRefused, HoldSkipped), the nodes of the held
// rows and the number of refused rows; the refused rows go to PlaceTLK.
func (e *Engine) HoldTL(j Jobs, kmax int, node, start []int32) ([]int32, int64, int64, error) {
	cnt := len(j.CPU)
	if kmax < 1 || kmax > MaxK {
		return nil, 0, 0, fmt.Errorf("fitgpu: kmax %d outside [1, %d]", kmax, MaxK)
	}
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(start)) || len(node) != cnt*kmax ||
		(len(j.NodesK) != 0 && len(j.NodesK) != cnt) {
		return nil, 0, 0, errLen
	}
	state := make([]int32, cnt)
	if cnt == 0 {
		return state, 0, 0, nil
	}
	var nk *C.uint16_t // NULL: every job took one node
	if len(j.NodesK) > 0 {
		nk = (*C.uint16_t)(unsafe.Pointer(&j.NodesK[0]))
	}
	var applied, refused C.int64_t
	rc := C.fit_hold_tl(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), nk, C.int32_t(kmax),
		(*C.int32_t)(unsafe.Pointer(&node[0])), (*C.int32_t)(unsafe.Pointer(&start[0])),
		(*C.int32_t)(unsafe.Pointer(&state[0])), &applied, &refused)
	runtime.KeepAlive(e)
	return state, int64(applied), int64(refused), check(rc)
}

// AdvanceTL moves the loaded timeline forward by a slots of slotMin minutes (DESIGN.md §2i): every
// node's timeline shifts left by a, and the a new slots at the far end take tailCPU / tailMemMiB /
// tailGPU of the node (caller's node order, values >= -1) wherever the node's last slot was usable:
// per node, its total minus the demand of the running jobs that end beyond the new horizon.  All
// three nil: every column continues its last slot, exact only when no reservation and no pending
// release reaches the old horizon edge.  Recorded placements follow with start' = max(start-a, 0)
// and wall' = (e-a-start')*slotMin, e = min(start+d, H); rows with e <= a are dropped.  a == 0 does
// nothing.
func (e *Engine) AdvanceTL(a int, tailCPU, tailMemMiB, tailGPU []int32) error {
	if a < 0 {
		return fmt.Errorf("fitgpu: a %d is negative", a)
	}
	if !sameLen(len(tailCPU), len(tailMemMiB), len(tailGPU)) {
		return errLen
	}
	var tc, tm, tg *C.int32_t // NULL: continue the last slot
	if len(tailCPU) > 0 {
		tc = (*C.int32_t)(unsafe.Pointer(&tailCPU[0]))
		tm = (*C.int32_t)(unsafe.Pointer(&tailMemMiB[0]))
		tg = (*C.int32_t)(unsafe.Pointer(&tailGPU[0]))
	}
	rc := C.fit_advance_tl(e.ctx, C.int32_t(a), tc, tm, tg)
	runtime.KeepAlive(e)
	return check(rc)
}

// Eta codes (fit_eta.code, include/fitgpu.h): when a job can start.  EtaPartition .. EtaNoNodes
// are WhyPartition .. WhyNoNodes.
const (
	EtaNow       = int32(C.FIT_ETA_NOW)
	EtaPartition = int32(C.FIT_ETA_PARTITION)
	EtaLimitTime = int32(C.FIT_ETA_LIMIT_TIME)
	EtaLimitCPUs = int32(C.FIT_ETA_LIMIT_CPUS)
	EtaLimitMem  = int32(C.FIT_ETA_LIMIT_MEM)
	EtaNoNodes   = int32(C.FIT_ETA_NO_NODES)
	EtaLater     = int32(C.FIT_ETA_LATER)
	EtaHorizon   = int32(C.FIT_ETA_HORIZON)
	EtaWindow    = int32(C.FIT_ETA_WINDOW) // fit_when_k_win only: no start inside the job's window
)

// Eta is one fit_eta row: the job judged alone against the current timeline (DESIGN.md §2d).
type Eta struct {
	Code    int32 // Eta*
	Dur     int32 // slots the job occupies: max(1, ceil(WallMin / slotMin))
	Start   int32 // earliest start slot over the partition's nodes, -1 if none
	Node    int32 // the node PlaceBackfill of this job alone would return, -1 if none
	WaitMin int32 // Start * slotMin, -1 if none
	Members int32 // schedulable nodes of the job's partition
	Hosts   int32 // members with a start inside the horizon
	Now     int32 // members that can start it at slot 0
}

func goEta(r *C.fit_eta) Eta {
	return Eta{Code: int32(r.code), Dur: int32(r.dur), Start: int32(r.start), Node: int32(r.node),
		WaitMin: int32(r.wait_min), Members: int32(r.members), Hosts: int32(r.hosts), Now: int32(r.now)}
}

// When gives every job, judged alone against the current timeline (LoadTimeline minus the
// reservations of every PlaceBackfill since), its earliest start and node (fit_when: `squeue
// --start`); it reserves nothing.  NodesK is not read: a backfill job takes one node.
func (e *Engine) When(j Jobs) ([]Eta, error) {
	cnt := len(j.CPU)
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part)) {
		return nil, errLen
	}
	if cnt == 0 {
		return nil, nil
	}
	rows := make([]C.fit_eta, cnt)
	rc := C.fit_when(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])), &rows[0])
	runtime.KeepAlive(e)
	if err := check(rc); err != nil {
		return nil, err
	}
	out := make([]Eta, cnt)
	for i := range rows {
		out[i] = goEta(&rows[i])
	}
	return out, nil
}

// WhenMessage is the row as one line (fit_when_message: "earliest start in 35 min (slot 7): 12/40
// nodes can run it inside the horizon, none now"); "" for a row with an unknown code.
func WhenMessage(t Eta) string {
	c := C.fit_eta{code: C.int32_t(t.Code), dur: C.int32_t(t.Dur), start: C.int32_t(t.Start),
		node: C.int32_t(t.Node), wait_min: C.int32_t(t.WaitMin), members: C.int32_t(t.Members),
		hosts: C.int32_t(t.Hosts), now: C.int32_t(t.Now)}
	buf := make([]byte, 256)
	n := C.fit_when_message(&c, (*C.char)(unsafe.Pointer(&buf[0])), C.int32_t(len(buf)))
	if n < 0 {
		return ""
	}
	return string(buf[:int(n)])
}

// Room codes (fit_room.code, include/fitgpu.h): how many more copies of a job fit now.
// RoomPartition .. RoomNoNodes are WhyPartition .. WhyNoNodes.
const (
	RoomSome      = int32(C.FIT_ROOM_SOME)
	RoomPartition = int32(C.FIT_ROOM_PARTITION)
	RoomLimitTime = int32(C.FIT_ROOM_LIMIT_TIME)
	RoomLimitCPUs = int32(C.FIT_ROOM_LIMIT_CPUS)
	RoomLimitMem  = int32(C.FIT_ROOM_LIMIT_MEM)
	RoomNoNodes   = int32(C.FIT_ROOM_NO_NODES)
	RoomNone      = int32(C.FIT_ROOM_NONE)
	RoomUnbounded = int32(C.FIT_ROOM_UNBOUNDED) // Best for a job that demands nothing
)

// Room is one fit_room row: the job judged alone against the current node table (DESIGN.md §2e).
type Room struct {
	Code     int32 // Room*
	Members  int32 // schedulable nodes of the job's partition
	Nodes    int32 // members the job fits now (Why.Fit)
	Best     int32 // the most copies one node takes, 0 if none
	Copies   int64 // copies over all members: Place of m one-node copies alone places min(m, Copies)
	BestNode int32 // a node that takes Best copies, the lowest id on a tie; -1 if none
	ByGPU    int32 // fitting members on which the GPUs run out first
	ByCPU    int32 // ... the cpus
	ByMem    int32 // ... the memory
}

func goRoom(r *C.struct_fit_room) Room {
	return Room{Code: int32(r.code), Members: int32(r.members), Nodes: int32(r.nodes), Best: int32(r.best),
		Copies: int64(r.copies), BestNode: int32(r.best_node), ByGPU: int32(r.by_gpu), ByCPU: int32(r.by_cpu),
		ByMem: int32(r.by_mem)}
}

// Room gives every job, judged alone against the current node table, the number of further copies
// of it that fit now and what limits them (fit_room); it changes nothing.  NodesK is not read: for
// a k-node job the row counts node shares.
func (e *Engine) Room(j Jobs) ([]Room, error) {
	cnt := len(j.CPU)
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part)) {
		return nil, errLen
	}
	if cnt == 0 {
		return nil, nil
	}
	rows := make([]C.struct_fit_room, cnt)
	rc := C.fit_room(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])), &rows[0])
	runtime.KeepAlive(e)
	if err := check(rc); err != nil {
		return nil, err
	}
	out := make([]Room, cnt)
	for i := range rows {
		out[i] = goRoom(&rows[i])
	}
	return out, nil
}

// RoomMessage is the row as one line (fit_room_message: "room for 12 more on 3/40 nodes (at most 5
// on one node): limited by gpu on 2, cpu on 1"); "" for a row with an unknown code.
func RoomMessage(r Room) string {
	c := C.struct_fit_room{code: C.int32_t(r.Code), members: C.int32_t(r.Members), nodes: C.int32_t(r.Nodes),
		best: C.int32_t(r.Best), copies: C.int64_t(r.Copies), best_node: C.int32_t(r.BestNode),
		by_gpu: C.int32_t(r.ByGPU), by_cpu: C.int32_t(r.ByCPU), by_mem: C.int32_t(r.ByMem)}
	buf := make([]byte, 256)
	n := C.fit_room_message(&c, (*C.char)(unsafe.Pointer(&buf[0])), C.int32_t(len(buf)))
	if n < 0 {
		return ""
	}
	return string(buf[:int(n)])
}

// Victims are the preemptible running jobs of each node, CSR by node id: node x's victims are
// [Off[x], Off[x+1]) in eviction order — Prio non-decreasing, the lowest first — each holding
// (CPU, MemMiB, GPU) on that node (DESIGN.md §2l).
type Victims struct {
	Off, Prio, CPU, MemMiB, GPU []int32
}

// LoadVictims hands the engine the running jobs Preempt may evict (fit_load_victims), after
// LoadNodes, which drops them.  An empty Off means no node has a victim.
func (e *Engine) LoadVictims(v Victims) error {
	if !sameLen(len(v.Prio), len(v.CPU), len(v.MemMiB), len(v.GPU)) {
		return errLen
	}
	if len(v.Off) == 0 {
		err := check(C.fit_load_victims(e.ctx, nil, nil, nil, nil, nil))
		runtime.KeepAlive(e)
		return err
	}
	if int(v.Off[len(v.Off)-1]) > len(v.Prio) {
		return fmt.Errorf("fitgpu: Off ends at %d but there are %d victims", v.Off[len(v.Off)-1], len(v.Prio))
	}
	var p, c, m, g *C.int32_t
	if len(v.Prio) > 0 {
		p, c = (*C.int32_t)(unsafe.Pointer(&v.Prio[0])), (*C.int32_t)(unsafe.Pointer(&v.CPU[0]))
		m, g = (*C.int32_t)(unsafe.Pointer(&v.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&v.GPU[0]))
	}
	err := check(C.fit_load_victims(e.ctx, (*C.int32_t)(unsafe.Pointer(&v.Off[0])), p, c, m, g))
	runtime.KeepAlive(e)
	return err
}

// Preempt codes (fit_evict.code, include/fitgpu.h): whether evicting running jobs makes a job fit.
// PrePartition .. PreNoNodes are WhyPartition .. WhyNoNodes.
const (
	PreFits      = int32(C.FIT_PRE_FITS)
	PrePartition = int32(C.FIT_PRE_PARTITION)
	PreLimitTime = int32(C.FIT_PRE_LIMIT_TIME)
	PreLimitCPUs = int32(C.FIT_PRE_LIMIT_CPUS)
	PreLimitMem  = int32(C.FIT_PRE_LIMIT_MEM)
	PreNoNodes   = int32(C.FIT_PRE_NO_NODES)
	PreEvict     = int32(C.FIT_PRE_EVICT)
	PreNone      = int32(C.FIT_PRE_NONE)
)

// Evict is one fit_evict row: the job judged alone against the current node table and the loaded
// victims (DESIGN.md §2l).  With Code == PreEvict the caller evicts the first Victims entries of
// Node's list, [Off[Node], Off[Node]+Victims), and the job fits Node.
type Evict struct {
	Code      int32 // Pre*
	Node      int32 // the chosen node, -1 if none
	Victims   int32 // entries of Node's list to evict, from its first; 0 unless PreEvict
	TopPrio   int32 // priority of the last of them, the highest evicted; 0 unless PreEvict
	Members   int32 // schedulable nodes of the job's partition
	Fit       int32 // members the job fits now (Why.Fit)
	Able      int32 // members a prefix of lower-priority victims frees
	Outranked int32 // members that only jobs of equal or higher priority hold
}

func goEvict(r *C.fit_evict) Evict {
	return Evict{Code: int32(r.code), Node: int32(r.node), Victims: int32(r.victims), TopPrio: int32(r.top_prio),
		Members: int32(r.members), Fit: int32(r.fit), Able: int32(r.able), Outranked: int32(r.outranked)}
}

// Preempt tells for every job, judged alone, whether it fits now, and if not which node to free
// and how many of its victims to evict (fit_preempt); it changes nothing and evicts nothing.  prio
// has one entry per job.  NodesK is not read: each job takes one node.
func (e *Engine) Preempt(j Jobs, prio []int32) ([]Evict, error) {
	cnt := len(j.CPU)
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part), len(prio)) {
		return nil, errLen
	}
	if cnt == 0 {
		return nil, nil
	}
	rows := make([]C.fit_evict, cnt)
	rc := C.fit_preempt(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])),
		(*C.int32_t)(unsafe.Pointer(&prio[0])), &rows[0])
	runtime.KeepAlive(e)
	if err := check(rc); err != nil {
		return nil, err
	}
	out := make([]Evict, cnt)
	for i := range rows {
		out[i] = goEvict(&rows[i])
	}
	return out, nil
}

// PreemptMessage is the row as one line (fit_preempt_message: "fits node 812 after evicting 2
// lower-priority jobs (highest priority 10): 37/512 nodes can be freed"); "" for a row with an
// unknown code.
func PreemptMessage(r Evict) string {
	c := C.fit_evict{code: C.int32_t(r.Code), node: C.int32_t(r.Node), victims: C.int32_t(r.Victims),
		top_prio: C.int32_t(r.TopPrio), members: C.int32_t(r.Members), fit: C.int32_t(r.Fit),
		able: C.int32_t(r.Able), outranked: C.int32_t(r.Outranked)}
	buf := make([]byte, 256)
	n := C.fit_preempt_message(&c, (*C.char)(unsafe.Pointer(&buf[0])), C.int32_t(len(buf)))
	if n < 0 {
		return ""
	}
	return string(buf[:int(n)])
}

// EvictK is one fit_evict_k row: the job judged alone on max(NodesK, 1) distinct nodes at once
// against the current node table and the loaded victims (DESIGN.md §2m).  Code is one of Pre*.
type EvictK struct {
	Code       int32 // Pre*: PreFits with Fit >= Need, PreEvict with Fit < Need <= Fit + Able, else PreNone
	Need       int32 // max(NodesK, 1)
	EvictNodes int32 // picks that need an eviction
	Victims    int32 // entries to evict, summed over the picks
	TopPrio    int32 // the highest priority evicted; 0 when EvictNodes == 0
	Members    int32 // as Evict
	Fit        int32
	Able       int32
	Outranked  int32
	Reserved   int32 // 0
}

func goEvictK(r *C.fit_evict_k) EvictK {
	return EvictK{Code: int32(r.code), Need: int32(r.need), EvictNodes: int32(r.evict_nodes), Victims: int32(r.victims),
		TopPrio: int32(r.top_prio), Members: int32(r.members), Fit: int32(r.fit), Able: int32(r.able),
		Outranked: int32(r.outranked), Reserved: int32(r.reserved)}
}

// PreemptK is Preempt for jobs of NodesK nodes (fit_preempt_k): for every job, judged alone, the Need
// nodes with the smallest keys — every node that fits now first, then the nodes whose eviction costs
// least.  nodes and victims have kmax entries per job: a PreFits or PreEvict row's picks in key order
// and the entries of each pick's list to evict, [Off[node], Off[node]+victims), 0 for a node that
// fits now; -1 and 0 elsewhere.  It changes nothing and evicts nothing.  prio has one entry per job;
// NodesK may be empty (every job takes one node).
func (e *Engine) PreemptK(j Jobs, prio []int32, kmax int) ([]EvictK, []int32, []int32, error) {
	cnt := len(j.CPU)
	if kmax < 1 || kmax > MaxK {
		return nil, nil, nil, fmt.Errorf("fitgpu: kmax %d outside [1, %d]", kmax, MaxK)
	}
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part), len(prio)) ||
		(len(j.NodesK) != 0 && len(j.NodesK) != cnt) {
		return nil, nil, nil, errLen
	}
	if cnt == 0 {
		return nil, nil, nil, nil
	}
	var nk *C.uint16_t // NULL: every job takes one node
	if len(j.NodesK) > 0 {
		nk = (*C.uint16_t)(unsafe.Pointer(&j.NodesK[0]))
	}
	rows := make([]C.fit_evict_k, cnt)
	nodes, victims := make([]int32, cnt*kmax), make([]int32, cnt*kmax)
	rc := C.fit_preempt_k(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])), nk,
		(*C.int32_t)(unsafe.Pointer(&prio[0])), C.int32_t(kmax), &rows[0],
		(*C.int32_t)(unsafe.Pointer(&nodes[0])), (*C.int32_t)(unsafe.Pointer(&victims[0])))
	runtime.KeepAlive(e)
	if err := check(rc); err != nil {
		return nil, nil, nil, err
	}
	out := make([]EvictK, cnt)
	for i := range rows {
		out[i] = goEvictK(&rows[i])
	}
	return out, nodes, victims, nil
}

// PreemptKMessage is the row as one line (fit_preempt_k_message: "fits 4 nodes after evicting 5
// lower-priority jobs on 3 of them (highest priority 10): 1 fit now, 37 can be freed, of 512 nodes");
// "" for a row with an unknown code.
func PreemptKMessage(r EvictK) string {
	c := C.fit_evict_k{code: C.int32_t(r.Code), need: C.int32_t(r.Need), evict_nodes: C.int32_t(r.EvictNodes),
		victims: C.int32_t(r.Victims), top_prio: C.int32_t(r.TopPrio), members: C.int32_t(r.Members),
		fit: C.int32_t(r.Fit), able: C.int32_t(r.Able), outranked: C.int32_t(r.Outranked),
		reserved: C.int32_t(r.Reserved)}
	buf := make([]byte, 256)
	n := C.fit_preempt_k_message(&c, (*C.char)(unsafe.Pointer(&buf[0])), C.int32_t(len(buf)))
	if n < 0 {
		return ""
	}
	return string(buf[:int(n)])
}

// VictimsTL are Victims for a loaded timeline (DESIGN.md §2n): End[k] is the slot at which the
// running job hands its resources back anyway, 0 <= End <= the horizon.  Evicting the entry frees
// what it holds on the slots [0, End) of its node.
type VictimsTL struct {
	Off, Prio, End, CPU, MemMiB, GPU []int32
}

// LoadVictimsTL hands the engine the running jobs PreemptTL may evict (fit_load_victims_tl), after
// LoadTimeline, which drops them; AdvanceTL keeps them and moves their ends along.  An empty Off
// means no node has a victim.
func (e *Engine) LoadVictimsTL(v VictimsTL) error {
	if !sameLen(len(v.Prio), len(v.End), len(v.CPU), len(v.MemMiB), len(v.GPU)) {
		return errLen
	}
	if len(v.Off) == 0 {
		err := check(C.fit_load_victims_tl(e.ctx, nil, nil, nil, nil, nil, nil))
		runtime.KeepAlive(e)
		return err
	}
	if int(v.Off[len(v.Off)-1]) > len(v.Prio) {
		return fmt.Errorf("fitgpu: Off ends at %d but there are %d victims", v.Off[len(v.Off)-1], len(v.Prio))
	}
	var p, d, c, m, g *C.int32_t
	if len(v.Prio) > 0 {
		p, d = (*C.int32_t)(unsafe.Pointer(&v.Prio[0])), (*C.int32_t)(unsafe.Pointer(&v.End[0]))
		c, m = (*C.int32_t)(unsafe.Pointer(&v.CPU[0])), (*C.int32_t)(unsafe.Pointer(&v.MemMiB[0]))
		g = (*C.int32_t)(unsafe.Pointer(&v.GPU[0]))
	}
	err := check(C.fit_load_victims_tl(e.ctx, (*C.int32_t)(unsafe.Pointer(&v.Off[0])), p, d, c, m, g))
	runtime.KeepAlive(e)
	return err
}

// PreemptTL is Preempt on the loaded timeline (fit_preempt_tl): every job judged alone, for a start
// now, against the current timeline — reservations included — and the victims of LoadVictimsTL.  The
// rows are Preempt's, PreemptMessage gives their text.  It changes nothing and evicts nothing.
func (e *Engine) PreemptTL(j Jobs, prio []int32) ([]Evict, error) {
	cnt := len(j.CPU)
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part), len(prio)) {
		return nil, errLen
	}
	if cnt == 0 {
		return nil, nil
	}
	rows := make([]C.fit_evict, cnt)
	rc := C.fit_preempt_tl(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])),
		(*C.int32_t)(unsafe.Pointer(&prio[0])), &rows[0])
	runtime.KeepAlive(e)
	if err := check(rc); err != nil {
		return nil, err
	}
	out := make([]Evict, cnt)
	for i := range rows {
		out[i] = goEvict(&rows[i])
	}
	return out, nil
}

// PreemptTLK is PreemptK on the loaded timeline (fit_preempt_tl_k): every job judged alone, for a start
// now on Need nodes at once, against the current timeline — reservations included — and the victims
// of LoadVictimsTL.  The rows, nodes and victims are PreemptK's, PreemptKMessage gives the rows' text.
// It changes nothing and evicts nothing.
func (e *Engine) PreemptTLK(j Jobs, prio []int32, kmax int) ([]EvictK, []int32, []int32, error) {
	cnt := len(j.CPU)
	if kmax < 1 || kmax > MaxK {
		return nil, nil, nil, fmt.Errorf("fitgpu: kmax %d outside [1, %d]", kmax, MaxK)
	}
	if !sameLen(cnt, len(j.MemMiB), len(j.GPU), len(j.WallMin), len(j.Part), len(prio)) ||
		(len(j.NodesK) != 0 && len(j.NodesK) != cnt) {
		return nil, nil, nil, errLen
	}
	if cnt == 0 {
		return nil, nil, nil, nil
	}
	var nk *C.uint16_t // NULL: every job takes one node
	if len(j.NodesK) > 0 {
		nk = (*C.uint16_t)(unsafe.Pointer(&j.NodesK[0]))
	}
	rows := make([]C.fit_evict_k, cnt)
	nodes, victims := make([]int32, cnt*kmax), make([]int32, cnt*kmax)
	rc := C.fit_preempt_tl_k(e.ctx, C.int32_t(cnt), (*C.int32_t)(unsafe.Pointer(&j.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&j.GPU[0])),
		(*C.int32_t)(unsafe.Pointer(&j.WallMin[0])), (*C.uint16_t)(unsafe.Pointer(&j.Part[0])), nk,
		(*C.int32_t)(unsafe.Pointer(&prio[0])), C.int32_t(kmax), &rows[0],
		(*C.int32_t)(unsafe.Pointer(&nodes[0])), (*C.int32_t)(unsafe.Pointer(&victims[0])))
	runtime.KeepAlive(e)
	if err := check(rc); err != nil {
		return nil, nil, nil, err
	}
	out := make([]EvictK, cnt)
	for i := range rows {
		out[i] = goEvictK(&rows[i])
	}
	return out, nodes, victims, nil
}

// EvictedTL reports evicted victims (fit_evicted_tl, DESIGN.md §2p): row i says that entry pos[i] of
// node[i]'s list — the caller's node id, the position in the list as it is before the call, 0 being
// the entry PreemptTL would evict first — is gone.  Its amounts go back to the slots [0, End) of its
// node, End as the queries read it, and the entry leaves the list; the timeline, the other entries and
// what AdvanceTL has moved them by stay loaded.  A victim that ran on several nodes is reported with
// one row per node, each position looked up in the caller's mirror of that node's list
// (ReadVictimsTL).  The engine evicts nothing: call it after the pods are deleted, then place the job
// with PlaceTLK.  A bad row — an unknown node, a position outside the list, a pair named twice —
// fails the whole call and changes nothing.
func (e *Engine) EvictedTL(node, pos []int32) error {
	if len(node) != len(pos) {
		return errLen
	}
	if len(node) == 0 {
		err := check(C.fit_evicted_tl(e.ctx, 0, nil, nil))
		runtime.KeepAlive(e)
		return err
	}
	rc := C.fit_evicted_tl(e.ctx, C.int32_t(len(node)), (*C.int32_t)(unsafe.Pointer(&node[0])),
		(*C.int32_t)(unsafe.Pointer(&pos[0])))
	runtime.KeepAlive(e)
	return check(rc)
}

// ReadVictimsTL returns the current lists by node id (fit_read_victims_tl): what LoadVictimsTL loaded,
// minus what EvictedTL has reported, every End as the queries read it now.  The list of a node in no
// partition is empty.  It changes nothing.
func (e *Engine) ReadVictimsTL() (VictimsTL, error) {
	v := VictimsTL{Off: make([]int32, e.nodes+1)}
	off := (*C.int32_t)(unsafe.Pointer(&v.Off[0]))
	rc := C.fit_read_victims_tl(e.ctx, off, 0, nil, nil, nil, nil, nil) // the offsets size the columns
	runtime.KeepAlive(e)
	if err := check(rc); err != nil {
		return VictimsTL{}, err
	}
	nv := int(v.Off[e.nodes])
	v.Prio, v.End, v.CPU = make([]int32, nv), make([]int32, nv), make([]int32, nv)
	v.MemMiB, v.GPU = make([]int32, nv), make([]int32, nv)
	if nv == 0 {
		return v, nil
	}
	rc = C.fit_read_victims_tl(e.ctx, off, C.int64_t(nv), (*C.int32_t)(unsafe.Pointer(&v.Prio[0])),
		(*C.int32_t)(unsafe.Pointer(&v.End[0])), (*C.int32_t)(unsafe.Pointer(&v.CPU[0])),
		(*C.int32_t)(unsafe.Pointer(&v.MemMiB[0])), (*C.int32_t)(unsafe.Pointer(&v.GPU[0])))
	runtime.KeepAlive(e)
	if err := check(rc); err != nil {
		return VictimsTL{}, err
	}
	return v, nil
}

// TLSet is one fit_set_tl row (DESIGN.md §2q): the slots [From, min(To, H)) of Node, the caller's node
// id, get the levels CPU, MemMiB and GPU, each >= -1; -1 closes the column.  From < 0: the row is
// skipped.  To = math.MaxInt32: to the horizon.
type TLSet struct {
	Node, From, To   int32
	CPU, MemMiB, GPU int32
}

// SetTL overwrites windows of the loaded timeline when a node changes outside the plan (fit_set_tl):
// it drains, resumes, gets a maintenance window, another avail_min or other totals.  Where rows
// overlap, the one with the largest index stands, so a resumed node is a base row over the whole
// horizon followed by the rows of its pending releases.  applied counts the live rows whose node has a
// run list, ignored those on a node that was loaded in no partition (it keeps reading -1: load a node
// that may come back with its partition bits and avail_min 0).  The node table, the victims' lists and
// what AdvanceTL has moved them by stay as they are.  A bad live row — an unknown node, From at or
// beyond the horizon, To <= From, a level below -1 — fails the whole call and changes nothing.
func (e *Engine) SetTL(rows []TLSet) (applied, ignored int64, err error) {
	var a, g C.int64_t
	m := len(rows)
	if m == 0 {
		err = check(C.fit_set_tl(e.ctx, 0, nil, nil, nil, nil, nil, nil, &a, &g))
		runtime.KeepAlive(e)
		return int64(a), int64(g), err
	}
	cols := make([]int32, 6*m) // node, from, to, cpu, mem, gpu: one column after another
	for i, r := range rows {
		cols[i], cols[m+i], cols[2*m+i] = r.Node, r.From, r.To
		cols[3*m+i], cols[4*m+i], cols[5*m+i] = r.CPU, r.MemMiB, r.GPU
	}
	col := func(k int) *C.int32_t { return (*C.int32_t)(unsafe.Pointer(&cols[k*m])) }
	rc := C.fit_set_tl(e.ctx, C.int32_t(m), col(0), col(1), col(2), col(3), col(4), col(5), &a, &g)
	runtime.KeepAlive(e)
	if err = check(rc); err != nil {
		return 0, 0, err
	}
	return int64(a), int64(g), nil
}

// Free is one fit_free row: the free capacity of one partition at one timeline slot, over the member
// nodes that are open there (DESIGN.md §2k).
type Free struct {
	CPU    int64 // free cpus, summed over the open members
	Mem    int64 // free MiB
	GPU    int64 // free GPUs
	Nodes  int32 // open member nodes at the slot
	MaxCPU int32 // the most free cpus on one of them, -1 when Nodes == 0: a one-node job that asks for
	MaxMem int32 // more cannot run at the slot; the three maxima may come from different nodes
	MaxGPU int32
}

func goFree(r *C.fit_free) Free {
	return Free{CPU: int64(r.cpu), Mem: int64(r.mem), GPU: int64(r.gpu), Nodes: int32(r.nodes),
		MaxCPU: int32(r.max_cpu), MaxMem: int32(r.max_mem), MaxGPU: int32(r.max_gpu)}
}

// FreeTL gives the free capacity of partitions 0 .. parts-1 (the node table's mask bits, 1..32 of
// them) at every slot of the loaded timeline, reservations included (fit_free_tl): out[p][t].  It
// changes nothing.  out[p][0] is the capacity now: while a timeline is loaded PartitionFree does
// not see the timeline's reservations.
func (e *Engine) FreeTL(parts int) ([][]Free, error) {
	if parts < 1 || parts > 32 {
		return nil, fmt.Errorf("fitgpu: parts %d outside 1..32", parts)
	}
	h := e.slots
	if h < 1 {
		h = 1 // no LoadTimeline yet: the library refuses the call before it writes a row
	}
	rows := make([]C.fit_free, parts*h)
	rc := C.fit_free_tl(e.ctx, C.int32_t(parts), &rows[0])
	runtime.KeepAlive(e)
	if err := check(rc); err != nil {
		return nil, err
	}
	out := make([][]Free, parts)
	for p := range out {
		out[p] = make([]Free, h)
		for t := range out[p] {
			out[p][t] = goFree(&rows[p*h+t])
		}
	}
	return out, nil
}

// FreeMessage is the row as one line (fit_free_message: "3 nodes open: 12 cpus, 3000 MiB, 2 gpus
// free (at most 8 cpus, 2000 MiB, 1 gpus on one node)", or "no open node").
func FreeMessage(r Free) string {
	c := C.fit_free{cpu: C.int64_t(r.CPU), mem: C.int64_t(r.Mem), gpu: C.int64_t(r.GPU), nodes: C.int32_t(r.Nodes),
		max_cpu: C.int32_t(r.MaxCPU), max_mem: C.int32_t(r.MaxMem), max_gpu: C.int32_t(r.MaxGPU)}
	buf := make([]byte, 256)
	n := C.fit_free_message(&c, (*C.char)(unsafe.Pointer(&buf[0])), C.int32_t(len(buf)))
	if n < 0 {
		return ""
	}
	return string(buf[:int(n)])
}

// IngestNodes turns `scontrol show nodes` output into the engine's node table (Client.Nodes +
// parseNode, pkg/slurm-agent/slurm.go:354-363 / parse.go:291-308, plus Gres/GresUsed, State,
// Partitions and NodeName), partitions[p] = the partition of part_mask bit p.
func IngestNodes(text string, partitions []string) (Nodes, []string, error) {
	ct := C.CString(text)
	defer C.free(unsafe.Pointer(ct))
	blob := make([]byte, 0, 64)
	for _, p := range partitions {
		blob = append(append(blob, p...), 0)
	}
	blob = append(blob, 0)
	cp := C.CBytes(blob)
	defer C.free(cp)
	capn := 2
	for i := 0; i+1 < len(text); i++ {
		if text[i] == '\n' && text[i+1] == '\n' {
			capn++
		}
	}
	n := Nodes{make([]int32, capn), make([]int32, capn), make([]int32, capn), make([]int32, capn),
		make([]uint32, capn)}
	names := make([]byte, len(text)+64)
	rc := C.fit_ingest_nodes(ct, (*C.char)(cp), C.int32_t(len(partitions)), C.int32_t(capn),
		(*C.int32_t)(unsafe.Pointer(&n.CPUFree[0])), (*C.int32_t)(unsafe.Pointer(&n.MemFreeMiB[0])),
		(*C.int32_t)(unsafe.Pointer(&n.GPUFree[0])), (*C.int32_t)(unsafe.Pointer(&n.AvailMin[0])),
		(*C.uint32_t)(unsafe.Pointer(&n.PartMask[0])), (*C.char)(unsafe.Pointer(&names[0])),
		C.int32_t(len(names)))
	if err := check(rc); err != nil {
		return Nodes{}, nil, err
	}
	cnt := int(rc)
	n = Nodes{n.CPUFree[:cnt], n.MemFreeMiB[:cnt], n.GPUFree[:cnt], n.AvailMin[:cnt], n.PartMask[:cnt]}
	out := make([]string, 0, cnt)
	for i, b := 0, 0; i < len(names) && len(out) < cnt; i++ {
		if names[i] == 0 {
			out = append(out, string(names[b:i]))
			b = i + 1
		}
	}
	return n, out, nil
}

// ---- CreatePod call site (include/fitgpu.h): every rule is in C; Go only marshals strings --------

// PodLabels holds the sbo.kubecluster.org/<key> label values newSubmitRequestForPod reads
// (pkg/slurm-virtual-kubelet/provider.go:74-123, keys pkg/common/labels.go:9-14); nil = absent.
type PodLabels struct {
	Nodes, CpusPerTask, MemPerCpu, NtasksPerNode, Array, Ntasks *string
}

func cstr(s *string) *C.char {
	if s == nil {
		return nil
	}
	return C.CString(*s)
}

// PodDemand derives a pod's admission requests from its labels and sbatch script (fit_pod_demand):
// the script's #SBATCH header under the labels, the operator's defaults, one request per array
// task that may run at once.
func PodDemand(l PodLabels, script string, part uint16, priority int64) ([]Demand, error) {
	fields := []*string{l.Nodes, l.CpusPerTask, l.MemPerCpu, l.NtasksPerNode, l.Array, l.Ntasks}
	cs := make([]*C.char, len(fields))
	for i, f := range fields {
		cs[i] = cstr(f)
		if cs[i] != nil {
			defer C.free(unsafe.Pointer(cs[i]))
		}
	}
	lab := C.fit_pod_labels{nodes: cs[0], cpus_per_task: cs[1], mem_per_cpu: cs[2],
		ntasks_per_node: cs[3], array: cs[4], ntasks: cs[5]}
	sc := C.CString(script)
	defer C.free(unsafe.Pointer(sc))
	n := C.fit_pod_demand(&lab, sc, C.uint16_t(part), C.int64_t(priority), nil, 0)
	if err := check(n); err != nil {
		return nil, err
	}
	reqs := make([]C.fit_admit_req, int(n))
	if err := check(C.fit_pod_demand(&lab, sc, C.uint16_t(part), C.int64_t(priority), &reqs[0], n)); err != nil {
		return nil, err
	}
	out := make([]Demand, len(reqs))
	for i, r := range reqs {
		out[i] = Demand{Priority: int64(r.priority), CPU: int32(r.cpu), MemMiB: int32(r.mem_mib),
			GPU: int32(r.gpu), WallMin: int32(r.wall_min), Part: uint16(r.part), NodesK: uint16(r.nodes_k),
			Flags: uint16(r.flags)}
	}
	return out, nil
}

// ScriptWithNodelist forwards the engine's nodes to slurmctld: the script with
// `#SBATCH --nodelist=` at the end of its #SBATCH header (fit_script_with_nodelist).
func ScriptWithNodelist(script string, names []string, nodes []int32) (string, error) {
	if len(nodes) == 0 {
		return script, nil
	}
	blob := nulJoin(names)
	cb := C.CBytes(blob)
	defer C.free(cb)
	sc := C.CString(script)
	defer C.free(unsafe.Pointer(sc))
	out := make([]byte, len(script)+32+len(blob)+1)
	rc := C.fit_script_with_nodelist(sc, (*C.char)(cb), C.int32_t(len(names)),
		(*C.int32_t)(unsafe.Pointer(&nodes[0])), C.int32_t(len(nodes)),
		(*C.char)(unsafe.Pointer(&out[0])), C.int32_t(len(out)))
	if err := check(rc); err != nil {
		return "", err
	}
	return string(out[:int(rc)]), nil
}

func nulJoin(names []string) []byte {
	blob := make([]byte, 0, 16*len(names)+1)
	for _, nm := range names {
		blob = append(append(blob, nm...), 0)
	}
	return append(blob, 0)
}

// NodeNames expands the Partition RPC's node list (parsePartition splits `Nodes=` on every comma,
// pkg/slurm-agent/parse.go:278-289) into the node names to send to the Nodes RPC: one engine row
// per name, record i of the answer is name i (fit_node_names).
func NodeNames(entries []string) ([]string, error) {
	if len(entries) == 0 {
		return []string{}, nil
	}
	cb := C.CBytes(nulJoin(entries))
	defer C.free(cb)
	for size := 1 << 16; ; size *= 16 {
		buf := make([]byte, size)
		n := C.fit_node_names((*C.char)(cb), C.int32_t(len(entries)), (*C.char)(unsafe.Pointer(&buf[0])),
			C.int32_t(size))
		if n == C.FIT_E_INVAL && size < 1<<24 {
			continue // buffer too small (a repeated name is FIT_E_PARSE: reported at once)
		}
		if err := check(n); err != nil {
			return nil, err
		}
		out := make([]string, 0, int(n))
		for b, i := 0, 0; len(out) < int(n); i++ {
			if buf[i] == 0 {
				out = append(out, string(buf[b:i]))
				b = i + 1
			}
		}
		return out, nil
	}
}

// SetMaxArraySize sets Slurm's MaxArraySize for PodDemand (process-wide); returns the previous value.
func SetMaxArraySize(n int32) (int32, error) {
	rc := C.fit_set_max_array_size(C.int32_t(n))
	if rc < 0 {
		return 0, check(C.int(rc))
	}
	return int32(rc), nil
}

// PartitionLimits converts a ResourcesResponse (workload.proto:137-148) into LoadPartitions' limits.
func PartitionLimits(wallTimeS, cpuPerNode, memPerNode int64) (maxTimeMin, maxCPUs, maxMemMiB int32, err error) {
	var t, c, m C.int32_t
	err = check(C.fit_partition_limits(C.int64_t(wallTimeS), C.int64_t(cpuPerNode), C.int64_t(memPerNode), &t, &c, &m))
	return int32(t), int32(c), int32(m), err
}

// ProtoNode is one workload.Node (workload.proto:165-174).
type ProtoNode struct {
	Cpus, Memory, Gpus, AlloCpus, AlloMemory, AlloGpus int64
}

// NodeColumns turns NodesResponse rows into a node table (free = total − alloc), every node in
// the partitions of partMask.
func NodeColumns(nodes []ProtoNode, partMask uint32) (Nodes, error) {
	n := len(nodes)
	t := Nodes{make([]int32, n), make([]int32, n), make([]int32, n), make([]int32, n), make([]uint32, n)}
	if n == 0 {
		return t, nil
	}
	rows := make([]C.fit_node, n)
	for i, x := range nodes {
		rows[i] = C.fit_node{cpus: C.int64_t(x.Cpus), memory: C.int64_t(x.Memory), gpus: C.int64_t(x.Gpus),
			allo_cpus: C.int64_t(x.AlloCpus), allo_memory: C.int64_t(x.AlloMemory), allo_gpus: C.int64_t(x.AlloGpus)}
	}
	rc := C.fit_node_columns(&rows[0], C.int32_t(n), C.uint32_t(partMask),
		(*C.int32_t)(unsafe.Pointer(&t.CPUFree[0])), (*C.int32_t)(unsafe.Pointer(&t.MemFreeMiB[0])),
		(*C.int32_t)(unsafe.Pointer(&t.GPUFree[0])), (*C.int32_t)(unsafe.Pointer(&t.AvailMin[0])),
		(*C.uint32_t)(unsafe.Pointer(&t.PartMask[0])))
	return t, check(rc)
}

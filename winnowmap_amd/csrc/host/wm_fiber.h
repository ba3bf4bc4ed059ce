// wm_fiber.h — cooperative fibers + the batching hub.
//
// The reference maps one read per thread with deeply data-dependent control flow (src/map.c:279-974: MCAS windows,
// MAPQ-gated retries, chain splitting). Rewriting that as explicit state machines is error-prone, so each unit of
// work (one stage-1 window position, one stage-2 pass) runs as a FIBER whose code reads sequentially; whenever it
// needs a device operation it files the request and yields.
//
// Execution model (one Hub per mapping call, T worker threads, no barriers):
//   * every worker owns the fibers of its reads and runs them until all of them wait for a device result;
//   * requests collect in the worker's local queues and are published to the Hub when the worker runs dry;
//   * a worker with nothing runnable becomes a DISPATCHER: it takes the whole pending queue of one operation type and
//     issues it as ONE batched device call (DeviceOps::*_batch — the call itself sleeps while the kernels run); several
//     dispatchers can be in flight at once (different operations, or the same one: DeviceOps::max_inflight()), so the
//     device always has queued work while the other workers keep running host glue;
//   * when a batch returns, the fibers that waited for it are handed back to their owners' inboxes.
// Queues grow while the device is busy and are taken whole, so batch sizes regulate themselves. Reads are admitted in a
// sliding window (the worker spawns a new read when one of its reads finishes), which keeps every stage of the path —
// sketch, seed, chain, align — in demand at the same time instead of in lock-step phases.
// Results do not depend on how requests are batched (every job is independent), so the output is deterministic.
//
// An OPERATION (OP_*) is one queue of requests of one type that one DeviceOps call serves. Everything about it that is data — the stem of its
// environment variables, its trace name, its scheduling defaults, the public report slot — is its row of op_table below; the hub's queues, counters
// and knobs are arrays indexed by OP_*. Adding one takes five steps, all in this file: the enum value, the table row, its place in stage_order
// (Scheduler::pick_locked), a typed filing method of Scheduler (the only way into a queue) and a `case` in Scheduler::dispatch (the only way out).
#pragma once
#if !defined(__x86_64__)
#include <ucontext.h>
#endif
#include <functional>
#include <exception>
#include <deque>
#include <vector>
#include <memory>
#include <mutex>
#include <condition_variable>
#include <atomic>
#include <stdlib.h>
#include <stdio.h>
#include <chrono>
#include <time.h>
#include "wm_ops.h"

namespace wm {

class Scheduler;
// Context switch. glibc's swapcontext saves and restores the signal mask with a system call on every switch (~200 ns; a read makes ~150
// switches); fibers never touch signal masks, so on x86-64 the switch is the textbook one: push the callee-saved registers, swap the stack
// pointers, pop, return. Other targets keep ucontext.
#if defined(__x86_64__)
extern "C" void wm_fiber_switch(void **save_sp, void *load_sp);
__asm__(
	".pushsection .text\n"
	".p2align 4\n"
	".globl wm_fiber_switch\n"
	".type wm_fiber_switch,@function\n"
	"wm_fiber_switch:\n"
	"	pushq %rbp\n	pushq %rbx\n	pushq %r12\n	pushq %r13\n	pushq %r14\n	pushq %r15\n"
	"	movq %rsp, (%rdi)\n"
	"	movq %rsi, %rsp\n"
	"	popq %r15\n	popq %r14\n	popq %r13\n	popq %r12\n	popq %rbx\n	popq %rbp\n"
	"	ret\n"
	".size wm_fiber_switch,.-wm_fiber_switch\n"
	".popsection\n");
struct FiberCtx { void *sp; };
#else
struct FiberCtx { ucontext_t uc; };
#endif
struct Fiber { FiberCtx ctx; char *stack; std::function<void()> fn; bool done; Scheduler *owner; int pending; };   // pending: batches this fiber still waits for
// OP_KSW_HEAVY: alignments whose single-wave run time is long (many rows x many lanes). They get their own queue so that the tail of a
// batch of heavy jobs (tens of milliseconds for ONE alignment) never delays the bulk of short gap fills.
// OP_KSW_HUGE: the few alignments that run for a large fraction of a second (unbanded fills across structural variants): a third queue,
// so that they do not hold back the heavy ones either.
// OP_WINDOW: one MCAS window / stage-2 pass, sketch → seed → sort → chain → extraction in one device call (WindowReq). The per-stage operations
// (OP_SKETCH / OP_SEED / OP_CHAIN) remain for callers that want a single stage.
// OP_WINDOW_BIG: the windows that can carry giant anchor sets — a stage-2 pass (handed-in anchors, or the whole read) — in a queue of their own: a
// window call lasts as long as its largest job (one 10^5-anchor sort + chain: ~25 ms), and the thousands of 1-kb stage-1 windows of a batch, which
// finish in one small kernel, would wait for it (round 4 timeline: gpurun_out/r04f).
// OP_EXTRA: the final scans of a read's regions (mm_update_extra's walk, ExtraReq), deferred to one request list per read when the switch is on (wm_ops.h).
// OP_FIX: mm_fix_cigar + that scan for regions that kept their stitched CIGAR (FixReq; the switch of wm_set_fix_device), batched the same way.
// OP_CS: the bodies of the cs:Z / MD:Z tags of a read's printed regions (CsReq; MM_F_OUT_CS / MM_F_OUT_MD with the switch of wm_set_cs_device), issued once the read's regions are final.
// OP_EQX: mm_update_cigar_eqx over a read's final CIGARs (EqxReq; MM_F_EQX with the switch of wm_set_eqx_device), issued after the read's OP_FIX / OP_EXTRA results are in.
enum { OP_SKETCH = 0, OP_SEED = 1, OP_CHAIN = 2, OP_KSW = 3, OP_KSW_HEAVY = 4, OP_KSW_HUGE = 5, OP_WINDOW = 6, OP_WINDOW_BIG = 7, OP_EXTRA = 8, OP_FIX = 9, OP_EQX = 10, OP_CS = 11, OP_N = 12 };
// What the hub knows about an operation that is not code, one row per OP_*:
//   env           stem of its scheduling variables WM_<env>_MIN_MORE / _MAX / _MIN_BATCH / _MAX_WAIT_MS (Hub::read_env);
//   name          what a WM_TRACE line calls it;
//   min_more, max_op    a further concurrent batch of an operation that is already in flight is issued when at least min_more requests are pending and fewer
//                 than max_op batches of it are running;
//   min_batch, max_wait_ms    a batch is worth its fixed cost — a kernel launch lasts at least as long as its longest job, and the device runs only so many
//                 kernels at once — when it is large: an operation is issued when min_batch requests are pending or the oldest has waited max_wait_ms,
//                 whichever comes first (0 / 0 = at once)
//                 (the huge queue: 512 jobs / 250 ms since round 5 — a launch of stripe-pipelined jobs lasts as long as its longest job whatever their number, so
//                 fewer, fuller launches: +3..9 % on config 2 together with the sixteen-wavefront routing, profiles/r05_sched.txt; before: 256 / 100 ms);
//   slot          which of the four public report slots (MapStats::n_batches / cpu_op / wall_op) its account is folded into: the heavy alignment queues and the
//                 deferred final passes are reported with the ksw operation, the fused window call in the first slot.
struct OpKnobs { size_t min_more; int max_op; size_t min_batch; double max_wait_ms; };
struct OpRow { int op; const char *env, *name; OpKnobs dflt; int slot; };
inline constexpr OpRow op_table[OP_N] = {
	{ OP_SKETCH,     "SKETCH",  "sketch",     {  4096, 2,  8192,  15 }, 0 },
	{ OP_SEED,       "SEED",    "seed",       {  4096, 2,  8192,  15 }, 1 },
	{ OP_CHAIN,      "CHAIN",   "chain",      {  4096, 2,  8192,  15 }, 2 },
	{ OP_KSW,        "KSW",     "ksw",        { 24576, 3, 98304,  30 }, 3 },
	{ OP_KSW_HEAVY,  "KSWH",    "ksw-heavy",  {  2048, 2, 12288,  60 }, 3 },
	{ OP_KSW_HUGE,   "KSWX",    "ksw-huge",   {    64, 1,   512, 250 }, 3 },
	{ OP_WINDOW,     "WINDOW",  "window",     {  4096, 3,  8192,  15 }, 0 },
	{ OP_WINDOW_BIG, "WINDOWB", "window-big", {  1024, 2,  2048,  30 }, 0 },
	{ OP_EXTRA,      "EXTRA",   "extra",      {  8192, 2,  4096,  15 }, 3 },
	{ OP_FIX,        "FIX",     "fix",        {  8192, 2,  4096,  15 }, 3 },
	{ OP_EQX,        "EQX",     "eqx",        {  8192, 2,  4096,  15 }, 3 },
	{ OP_CS,         "CS",      "cs",         {  8192, 2,  4096,  15 }, 3 },
};
constexpr bool op_table_in_order(int i = 0) { return i == OP_N || (op_table[i].op == i && op_table_in_order(i + 1)); }
static_assert(op_table_in_order(), "op_table: row i describes operation i");
inline double thread_cpu_s() { timespec ts; clock_gettime(CLOCK_THREAD_CPUTIME_ID, &ts); return (double)ts.tv_sec + 1e-9 * (double)ts.tv_nsec; }
inline double wall_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// a host-side loop of a batched call that idle workers help with (ParHook, wm_core.h)
struct HelpTask { const std::function<void(size_t)> *fn; size_t n, chunk; std::atomic<size_t> next; int helpers; const char *site; std::exception_ptr err; std::mutex err_mu; };

struct Hub {
	Hub(DeviceOps *ops_, const wm_ksw_score_t &sc_, int w_, int k_) : ops(ops_), sc(sc_), w(w_), k(k_) { max_inflight = ops->max_inflight(); if (max_inflight < 1) max_inflight = 1; read_env(); par.H = this; }
	DeviceOps *ops;
	wm_ksw_score_t sc;
	int w, k;
	int max_inflight;                       // batched device calls that may run concurrently (device contexts of the ops object)
	bool splice = false; int noncan = 0, junc_bonus = 0;     // MM_F_SPLICE: alignments go through DeviceOps::exts2_batch with these (src/align.c:326-327)
	int64_t max_sw_mat = 0;                 // mm_mapopt_t::max_sw_mat (--cap-sw-mat): pairs with more DP cells are not aligned (src/align.c:323-325)
	std::mutex mu;
	std::condition_variable cv;
	// published requests and the fibers waiting for them (taken whole by a dispatcher). A queue holds the requests of ONE type: only the typed filing
	// methods of Scheduler put anything in, and Scheduler::dispatch gives every operation's queue its type back
	std::vector<void*> q[OP_N];
	bool fix_dev = false;                   // ... and mm_fix_cigar with them, to DeviceOps::fix_extra_batch (fix_device_on() when the call started)
	bool eqx_dev = false;                   // ... and, under MM_F_EQX, the = / X rewriting after them, to DeviceOps::eqx_batch (eqx_device_on() when the call started)
	bool cs_dev = false;                    // ... and, under MM_F_OUT_CS / MM_F_OUT_MD, the tags' bodies of a finished read to DeviceOps::cs_batch (cs_device_on() when the call started)
	bool ll_dev = false;                    // the callers of ksw_ll_i16 file local-score requests (KswReq::local) in the alignment queue (ll_device_on() when the call started)
	bool extra_dev = false;                 // the mapping call defers its regions' final scans to DeviceOps::extra_batch (extra_device_on() when the call started)
	std::vector<Fiber*> waiters[OP_N];
	int inflight = 0, inflight_op[OP_N] = {};
	int n_workers = 1, n_idle = 0;          // workers of the mapping call; workers asleep with nothing runnable
	std::vector<HelpTask*> help;            // loops of running batched calls that still have chunks to hand out
	double cpu_help = 0;                    // CPU seconds idle workers spent inside such loops
	std::vector<std::pair<const char*, double>> site_cpu;   // ... and the CPU seconds of every labelled loop (WM_SITE), dispatcher + helpers
	void add_site(const char *site, double s) { if (!site) site = "(unlabelled)"; for (auto &e : site_cpu) if (e.first == site) { e.second += s; return; } site_cpu.emplace_back(site, s); }
	// an exception in the loop body (staging buffers throw bad_alloc) is kept — the first one — and rethrown by the call's owner after every helper
	// has left; the remaining chunks are skipped (a helper thread must never unwind into std::terminate, nor leave `helpers` raised)
	static void help_work(HelpTask &t)
	{
		try {
			for (;;) { const size_t b = t.next.fetch_add(t.chunk); if (b >= t.n) break; const size_t e = b + t.chunk < t.n ? b + t.chunk : t.n; for (size_t i = b; i < e; ++i) (*t.fn)(i); }
		} catch (...) {
			std::lock_guard<std::mutex> lk(t.err_mu);
			if (!t.err) t.err = std::current_exception();
			t.next.store(t.n);
		}
	}
	// the hook a dispatching worker installs around its batched call: the loop is shared with whoever is idle
	struct Par : ParHook {
		Hub *H;
		void run(size_t n, const std::function<void(size_t)> &fn) override
		{
			HelpTask t;
			t.fn = &fn; t.n = n; t.next.store(0); t.helpers = 0; t.site = tl_par_site(); tl_par_site() = 0;
			t.chunk = n / (size_t)(4 * (H->n_workers > 0 ? H->n_workers : 1));
			if (t.chunk < 16) t.chunk = 16;
			if (tl_par_chunk()) { t.chunk = tl_par_chunk(); tl_par_chunk() = 0; }         // (coarse tasks: parallel_tasks)
			{ std::lock_guard<std::mutex> lk(H->mu); H->help.push_back(&t); }
			H->cv.notify_all();
			const double c0 = thread_cpu_s();
			help_work(t);
			const double dc = thread_cpu_s() - c0;
			std::unique_lock<std::mutex> lk(H->mu);
			H->add_site(t.site, dc);
			for (size_t i = 0; i < H->help.size(); ++i) if (H->help[i] == &t) { H->help.erase(H->help.begin() + i); break; }
			while (t.helpers > 0) H->cv.wait(lk);          // (helpers announce themselves and leave under the hub mutex)
			lk.unlock();
			if (t.err) std::rethrow_exception(t.err);      // (the task is deregistered and nobody refers to this frame any more)
		}
	} par;
	std::atomic<int64_t> live{0};           // fibers alive + reads not yet admitted, over all workers: 0 = the mapping call is finished
	uint64_t n_batches[OP_N] = {}, n_reqs[OP_N] = {};
	// where the host time goes (seconds, summed over the workers): CPU time running fibers, CPU and wall time inside the batched
	// calls per operation, wall time asleep waiting for results
	double cpu_fiber = 0, cpu_op[OP_N] = {}, wall_op[OP_N] = {}, wall_idle = 0;
	double wall_fiber = 0, wall_lock = 0, wall_total = 0;     // wall time running fibers (>> cpu_fiber: the workers are being descheduled), waiting for the hub mutex, inside run()
	size_t pending(int op) const { return q[op].size(); }
	OpKnobs knob[OP_N];                     // scheduling knobs: the defaults of op_table, overridden by the environment (read once per mapping call)
	double first_pending[OP_N] = {};        // wall_s() when the queue of the operation last became non-empty
	long heavy_units = 8192;                // rows x 128-lane register pairs above which an alignment goes to the heavy queue (0 = no heavy queue)
	long huge_units = 131072;               // ... and to the queue of the few very long ones (0 = none)
	void read_env()
	{
		for (int op = 0; op < OP_N; ++op) {
			OpKnobs &kn = knob[op] = op_table[op].dflt;
			char key[64];
			snprintf(key, sizeof(key), "WM_%s_MIN_MORE", op_table[op].env); if (getenv(key)) kn.min_more = (size_t)atol(getenv(key));
			snprintf(key, sizeof(key), "WM_%s_MAX", op_table[op].env); if (getenv(key)) kn.max_op = atoi(getenv(key));
			snprintf(key, sizeof(key), "WM_%s_MIN_BATCH", op_table[op].env); if (getenv(key)) kn.min_batch = (size_t)atol(getenv(key));
			snprintf(key, sizeof(key), "WM_%s_MAX_WAIT_MS", op_table[op].env); if (getenv(key)) kn.max_wait_ms = atof(getenv(key));
		}
		if (getenv("WM_KSW_HEAVY_UNITS")) heavy_units = atol(getenv("WM_KSW_HEAVY_UNITS"));
		if (getenv("WM_KSW_HUGE_UNITS")) huge_units = atol(getenv("WM_KSW_HUGE_UNITS"));
	}
};

class Scheduler {
public:
	explicit Scheduler(Hub *hub, int rank = 0) : hub_(hub), rank_(rank) {}
	~Scheduler() { for (Fiber *f : pool_) delete f; for (char *sl : slabs_) free(sl); }

	void spawn(std::function<void()> fn)
	{
		Fiber *f;
		if (!pool_.empty()) { f = pool_.back(); pool_.pop_back(); }
		else {           // stacks come from slabs of 64 (one mapping per slab: a window of 10^4..10^5 reads x ~10 fibers would otherwise need that many mappings)
			if (slab_left_ == 0) { slabs_.push_back((char*)malloc(kStack * kSlab)); slab_left_ = kSlab; }
			f = new Fiber(); f->stack = slabs_.back() + kStack * (size_t)(kSlab - slab_left_--);
		}
		f->fn = std::move(fn); f->done = false;
#if defined(__x86_64__)
		{   // a fresh stack that "returns" into the trampoline: six zeroed callee-saved registers, then the entry address; the slot above it
			// keeps the stack 16-byte aligned at the trampoline's entry as the ABI expects after a call
			void **top = (void**)(((uintptr_t)f->stack + kStack) & ~(uintptr_t)15);
			top[-1] = 0;
			top[-2] = (void*)&Scheduler::trampoline;
			for (int i = 3; i <= 8; ++i) top[-i] = 0;
			f->ctx.sp = (void*)(top - 8);
		}
#else
		getcontext(&f->ctx.uc);
		f->ctx.uc.uc_stack.ss_sp = f->stack; f->ctx.uc.uc_stack.ss_size = kStack; f->ctx.uc.uc_link = &main_.uc;
		const uintptr_t p = (uintptr_t)f;
		makecontext(&f->ctx.uc, (void (*)())&Scheduler::entry, 3, (unsigned)(p & 0xffffffffu), (unsigned)(p >> 32), 0);
#endif
		f->owner = this;
		ready_.push_back(f);
		hub_->live.fetch_add(1);
	}
	// work that is not a fiber yet (reads waiting for admission) also keeps the mapping call alive
	void hold(int64_t n) { hub_->live.fetch_add(n); }
	void release(int64_t n) { hub_->live.fetch_sub(n); }

	// run until the whole mapping call (all workers) has finished
	void run()
	{
		Hub &H = *hub_;
		double cpu_fiber = 0, wall_idle = 0, wall_fiber = 0, wall_lock = 0;
		const double run_w0 = wall_s();
#if defined(__x86_64__)
		tl_running() = this;
#endif
		for (;;) {
			const double c0 = thread_cpu_s(), fw0 = wall_s();
			while (!ready_.empty()) {
				cur_ = ready_.front(); ready_.pop_front();
				switch_to(main_, cur_->ctx);
				if (cur_->done) { cur_->fn = nullptr; pool_.push_back(cur_); H.live.fetch_sub(1); }
				cur_ = 0;
			}
			cpu_fiber += thread_cpu_s() - c0;
			const double lw0 = wall_s();
			wall_fiber += lw0 - fw0;
			std::unique_lock<std::mutex> lk(H.mu);
			wall_lock += wall_s() - lw0;
			publish_locked();
			for (;;) {
				if (!inbox_.empty()) { for (Fiber *f : inbox_) ready_.push_back(f); inbox_.clear(); break; }
				if (H.live.load() == 0) { H.cpu_fiber += cpu_fiber; H.wall_idle += wall_idle; H.wall_fiber += wall_fiber; H.wall_lock += wall_lock; H.wall_total += wall_s() - run_w0; H.cv.notify_all(); return; }
				double wake_in = 1e9;
				const int op = pick_locked(&wake_in);
				if (op >= 0) { dispatch(op, lk); continue; }      // (returns with the lock held again)
				{   // nothing to issue: lend a hand to a running batched call's host-side loop
					HelpTask *ht = 0;
					for (HelpTask *t : H.help) if (t->next.load() < t->n) { ht = t; break; }
					if (ht) {
						++ht->helpers;
						lk.unlock();
						const double hc0 = thread_cpu_s();
						Hub::help_work(*ht);
						const double hc = thread_cpu_s() - hc0;
						lk.lock();
						H.cpu_help += hc; H.add_site(ht->site, hc);
						if (--ht->helpers == 0) H.cv.notify_all();
						continue;
					}
				}
				const double w0 = wall_s();
				++H.n_idle;
				if (wake_in > 0.5) wake_in = 0.5;                  // (also re-checks the drain condition)
				H.cv.wait_for(lk, std::chrono::duration<double>(wake_in < 2e-4 ? 2e-4 : wake_in));
				--H.n_idle;
				wall_idle += wall_s() - w0;
			}
		}
	}

	// ---- called from inside a fiber ----
	void sketch(SketchReq &r) { l_q_[OP_SKETCH].push_back(&r); wait(1 << OP_SKETCH); }
	void seed(SeedReq &r) { l_q_[OP_SEED].push_back(&r); wait(1 << OP_SEED); }
	void chain(ChainReq &r) { l_q_[OP_CHAIN].push_back(&r); wait(1 << OP_CHAIN); }
	void window(WindowReq &r)
	{
		// WM_WINDOW_BIG_LEN=8192 switches the second queue on (stage-1 windows are at most maxPrefixLength long: 8 000 for map-ont). Off by default: measured
		// neutral (0.242 vs 0.247 Gbp/s, profiles/r04g_sched_sweep.txt) — even a window call of a dozen requests takes 50-90 ms, waiting for a device context
		static const int big_len = getenv("WM_WINDOW_BIG_LEN") ? atoi(getenv("WM_WINDOW_BIG_LEN")) : -1;
		const bool big = big_len >= 0 && (!r.pre.empty() || r.len > big_len);
		const int op = big ? OP_WINDOW_BIG : OP_WINDOW;
		l_q_[op].push_back(&r);
		wait(1 << op);
	}
	void ksw(std::vector<KswReq> &rs)
	{
		if (rs.empty()) return;
		int ops = 0;
		const long hu = hub_->heavy_units, xu = hub_->huge_units;
		for (KswReq &r : rs) {
			if (r.local) { l_q_[OP_KSW].push_back(&r); ops |= 1 << OP_KSW; continue; }      // a local score: no band to classify by, and --cap-sw-mat does not apply (src/align.c:78, :539, :824)
			if (hub_->max_sw_mat > 0 && (int64_t)r.tlen() * r.qlen() > hub_->max_sw_mat) {      // --cap-sw-mat (src/align.c:323-325): not aligned, reported as z-dropped
				r.ez = wm_ksw_result_t(); r.ez.max_q = r.ez.max_t = r.ez.mqe_t = r.ez.mte_q = -1; r.ez.score = r.ez.mqe = r.ez.mte = -0x40000000; r.ez.zdropped = 1;
				r.cigar.clear();
				continue;
			}
			const long un = ksw_units(r);
			const int op = hub_->splice ? OP_KSW : xu > 0 && un > xu ? OP_KSW_HUGE : hu > 0 && un > hu ? OP_KSW_HEAVY : OP_KSW;   // (splice mode: one queue, exts2 has no band to classify by)
			l_q_[op].push_back(&r);
			ops |= 1 << op;
		}
		if (ops) wait(ops);
	}
	// the callers of ksw_ll_i16 file their jobs as local-score requests through ksw() instead of running them inside the fiber
	bool ll_deferred() const { return hub_->ll_dev; }
	// the deferred final scans of one read's regions (ExtraReq): one batched request, served together with those of the other reads in flight
	bool extra_deferred() const { return hub_->extra_dev; }
	void extra(std::vector<ExtraReq> &rs)
	{
		if (rs.empty()) return;
		for (ExtraReq &r : rs) l_q_[OP_EXTRA].push_back(&r);
		wait(1 << OP_EXTRA);
	}
	// ... and of the regions whose mm_fix_cigar waits too (FixReq), together with the scan-only ones of the same read: one wait for both lists
	bool fix_deferred() const { return hub_->fix_dev; }
	void fix_extra(std::vector<FixReq> &fs, std::vector<ExtraReq> &rs)
	{
		if (fs.empty()) { extra(rs); return; }
		for (FixReq &r : fs) l_q_[OP_FIX].push_back(&r);
		for (ExtraReq &r : rs) l_q_[OP_EXTRA].push_back(&r);
		wait(1 << OP_FIX | (rs.empty() ? 0 : 1 << OP_EXTRA));
	}
	// ... and, once those results are in, the = / X rewriting of the read's final CIGARs (EqxReq)
	bool eqx_deferred() const { return hub_->eqx_dev; }
	void eqx(std::vector<EqxReq> &rs)
	{
		if (rs.empty()) return;
		for (EqxReq &r : rs) l_q_[OP_EQX].push_back(&r);
		wait(1 << OP_EQX);
	}
	// ... and, when the read's regions are final, the bodies of their cs:Z / MD:Z tags (CsReq)
	bool cs_deferred() const { return hub_->cs_dev; }
	void cs(std::vector<CsReq> &rs)
	{
		if (rs.empty()) return;
		for (CsReq &r : rs) l_q_[OP_CS].push_back(&r);
		wait(1 << OP_CS);
	}
	// serial work of one alignment on its wavefront: anti-diagonals x 128-lane register pairs of the band hull
	static long ksw_units(const KswReq &r)
	{
		const long ql = (long)r.qlen(), tl = (long)r.tlen();
		long w = r.w < 0 ? (ql > tl ? ql : tl) : r.w, n = ql < tl ? ql : tl;
		if (n > w + 1) n = w + 1;
		return (ql + tl) * ((n + 127) / 128 + 1);
	}

private:
	static constexpr size_t kStack = 256 * 1024;
	static constexpr int kSlab = 64;
#if defined(__x86_64__)
	static Scheduler *&tl_running() { static thread_local Scheduler *s = 0; return s; }
	static void switch_to(FiberCtx &from, FiberCtx &to) { wm_fiber_switch(&from.sp, to.sp); }
	static void trampoline()                // first activation of a fiber: runs on the fiber's own stack, never returns
	{
		Scheduler *self = tl_running();
		Fiber *f = self->cur_;
		f->fn();
		f->done = true;
		self = tl_running();                // (the fiber may have been resumed by the same worker only: owners do not migrate)
		switch_to(f->ctx, self->main_);
		__builtin_trap();
	}
#else
	static void switch_to(FiberCtx &from, FiberCtx &to) { swapcontext(&from.uc, &to.uc); }
	static void entry(unsigned lo, unsigned hi, unsigned)
	{
		Fiber *f = (Fiber*)((uintptr_t)lo | (uintptr_t)hi << 32);
		f->fn();
		f->done = true;                     // uc_link returns to the scheduler
	}
#endif
	void wait(int ops)                      // ops: bit set of the operations this fiber filed requests for
	{
		Fiber *me = cur_;
		me->pending = 0;
		for (int op = 0; op < OP_N; ++op) if (ops >> op & 1) { l_wait_[op].push_back(me); ++me->pending; }
		switch_to(me->ctx, main_);
	}
	void publish_locked()
	{
		Hub &H = *hub_;
		bool any = false;
		const double now = wall_s();
		for (int op = 0; op < OP_N; ++op) if (H.pending(op) == 0) H.first_pending[op] = now;     // (stamps queues that are about to become non-empty)
		for (int op = 0; op < OP_N; ++op) {
			if (!l_q_[op].empty()) { H.q[op].insert(H.q[op].end(), l_q_[op].begin(), l_q_[op].end()); l_q_[op].clear(); any = true; }
			if (!l_wait_[op].empty()) { H.waiters[op].insert(H.waiters[op].end(), l_wait_[op].begin(), l_wait_[op].end()); l_wait_[op].clear(); }
		}
		if (any) H.cv.notify_all();          // somebody idle may want to dispatch what was just published
	}
	// which operation this idle worker should issue now (-1: none). An operation with nothing in flight goes first (keeps every stage
	// of the path moving); a further concurrent batch of the same operation is only worth its fixed cost when the queue is large.
	int pick_locked(double *wake_in_s)
	{
		Hub &H = *hub_;
		*wake_in_s = 1e9;
		if (H.inflight >= H.max_inflight) return -1;
		const double now = wall_s();
		// nothing running anywhere and nobody able to produce more requests: whatever is pending must go now
		const bool drain = H.inflight == 0 && H.n_idle + 1 >= H.n_workers;
		int best = -1;
		static const int stage_order[OP_N] = { OP_CS, OP_EQX, OP_FIX, OP_EXTRA, OP_KSW_HUGE, OP_KSW_HEAVY, OP_KSW, OP_WINDOW_BIG, OP_CHAIN, OP_SEED, OP_SKETCH, OP_WINDOW };
		for (int oi = 0; oi < OP_N; ++oi) {                   // later stages first: finishing reads frees their memory and admits new ones
			const int op = stage_order[oi];
			const size_t n = H.pending(op);
			if (n == 0) continue;
			const double waited_ms = (now - H.first_pending[op]) * 1e3;
			const bool ripe = drain || n >= H.knob[op].min_batch || waited_ms >= H.knob[op].max_wait_ms;
			if (!ripe) { const double left = (H.knob[op].max_wait_ms - waited_ms) * 1e-3; if (left < *wake_in_s) *wake_in_s = left; continue; }
			if (H.inflight_op[op] == 0) return op;
			if (n >= H.knob[op].min_more && H.inflight_op[op] < H.knob[op].max_op && best < 0) best = op;
		}
		return best;
	}
	template <class R> static std::vector<R*> typed(const std::vector<void*> &q) { std::vector<R*> v; v.reserve(q.size()); for (void *p : q) v.push_back(static_cast<R*>(p)); return v; }
	void dispatch(int op, std::unique_lock<std::mutex> &lk)
	{
		Hub &H = *hub_;
		std::vector<Fiber*> waiters;
		waiters.swap(H.waiters[op]);
		std::vector<void*> q;
		q.swap(H.q[op]);
		const size_t n = q.size();
		++H.inflight; ++H.inflight_op[op]; ++H.n_batches[op]; H.n_reqs[op] += n;
		lk.unlock();
		static const bool trace = getenv("WM_TRACE") != 0;
		const auto t0 = std::chrono::steady_clock::now();
		const double c0 = thread_cpu_s(), w0 = wall_s();
		ParHook *const prev_hook = tl_par_hook();
		tl_par_hook() = &H.par;
		try {
			switch (op) {          // the queue gets its type back: what the filing method of this operation put in
			case OP_SKETCH: { auto a = typed<SketchReq>(q); H.ops->sketch_batch(H.w, H.k, a); break; }
			case OP_SEED: { auto b = typed<SeedReq>(q); H.ops->seed_batch(b); break; }
			case OP_CHAIN: { auto c = typed<ChainReq>(q); H.ops->chain_batch(c); break; }
			case OP_KSW: case OP_KSW_HEAVY: case OP_KSW_HUGE: {
				auto d = typed<KswReq>(q);
				std::vector<KswReq*> loc;                   // the local-score requests among them (only with the switch of wm_set_ll_device on) go to their own call
				if (H.ll_dev) for (KswReq *r : d) if (r->local) loc.push_back(r);      // (switch off: nobody files one, and the queue is not walked)
				if (!loc.empty()) {
					size_t k = 0;
					for (KswReq *r : d) if (!r->local) d[k++] = r;
					d.resize(k);
					int8_t mat[25];                             // ksw_gen_simple_mat (src/align.c:9-22) of the call's scores
					for (int i = 0; i < 25; ++i) mat[i] = (i / 5 == 4 || i % 5 == 4) ? H.sc.sc_ambi : i / 5 == i % 5 ? H.sc.match : H.sc.mismatch;
					H.ops->ll_batch(mat, H.sc.q, H.sc.e, loc);
					if (d.empty()) break;
				}
				if (H.splice) H.ops->exts2_batch(H.sc, H.noncan, H.junc_bonus, d);
				else H.ops->ksw_batch(H.sc, d);
				break;
			}
			case OP_WINDOW: case OP_WINDOW_BIG: { auto wq = typed<WindowReq>(q); H.ops->window_batch(H.w, H.k, wq); break; }
			case OP_EXTRA: { auto xq = typed<ExtraReq>(q); if (!xq.empty()) H.ops->extra_batch(xq[0]->sc, xq); break; }      // (one score per mapping call)
			case OP_FIX: { auto fq = typed<FixReq>(q); if (!fq.empty()) H.ops->fix_extra_batch(fq[0]->sc, fq); break; }
			case OP_EQX: { auto eq = typed<EqxReq>(q); if (!eq.empty()) H.ops->eqx_batch(eq); break; }
			case OP_CS: { auto cq = typed<CsReq>(q); if (!cq.empty()) H.ops->cs_batch(cq); break; }
			}
		} catch (const std::exception &e) {          // the waiters below are released in any case (their requests keep their zero-initialised results)
			note_internal_error(e.what(), __FILE__, __LINE__);
		} catch (...) {
			note_internal_error("exception in a batched device call", __FILE__, __LINE__);
		}
		if (trace) fprintf(stderr, "[batch] worker %2d %s n=%zu %.1f ms\n", rank_, op_table[op].name, n,
		                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
		tl_par_hook() = prev_hook;
		const double dc = thread_cpu_s() - c0, dw = wall_s() - w0;
		lk.lock();
		H.cpu_op[op] += dc; H.wall_op[op] += dw;
		--H.inflight; --H.inflight_op[op];
		for (Fiber *f : waiters)
			if (--f->pending == 0) f->owner->inbox_.push_back(f);      // (counters and inboxes are protected by the hub mutex)
		H.cv.notify_all();
	}

	Hub *hub_;
	int rank_;
	FiberCtx main_;
	Fiber *cur_ = 0;
	std::deque<Fiber*> ready_;
	std::vector<Fiber*> pool_;
	std::vector<char*> slabs_; int slab_left_ = 0;
	std::vector<Fiber*> inbox_;             // fibers whose results arrived (filled by dispatchers under the hub mutex)
	std::vector<void*> l_q_[OP_N];          // requests filed since the last publish, per operation (the types of Hub::q)
	std::vector<Fiber*> l_wait_[OP_N];
};

} // namespace wm

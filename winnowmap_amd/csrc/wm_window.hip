// wm_window.hip — libwmgpu.so, window unit: one MCAS window / stage-2 pass on the device in ONE call, nothing leaves HBM in between — sketch (mm_sketch)
// -> seed (collect_seed_hits) -> sort (radix_sort_128x) -> chain fill + extraction (mm_chain_dp): window_kernel.h, seedchain_kernel.h; wm_window_batch of include/wm_gpu.h.
#include "wm_rt.h"
#include "simt.h"
#include "reads2bit.h"
#include "sketch_kernel.h"
#include "seedchain_kernel.h"
#include "window_kernel.h"
#include "chain_fill.h"
#include "sdust_kernel.h"
#include "host/wm_core.h"
#include "host/wm_sdust.h"

// ======================================================================================================
// -T: the SDUST intervals of a sequence and the squeeze of its minimizers (sdust_kernel.h; mm_dust_minier, src/map.c:43-67)
// ======================================================================================================
// entries of the list of perfect intervals a wavefront keeps in LDS; WM_SDUST_CAP in the environment (64 .. the compiled size) shrinks it so that the
// tests reach the path on which the host finishes a job. Read per call.
static int sdust_list_cap()
{
	const char *e = getenv("WM_SDUST_CAP");
	const int v = e ? atoi(e) : WM_SDUST_CAP;
	return v < 64 ? 64 : v > WM_SDUST_CAP ? WM_SDUST_CAP : v;
}
// process-wide account of the filter (wm_sdust_stats): window calls that ran it, microseconds of win_dust_kernel, jobs it saw, jobs the host finished, largest list
static std::atomic<uint64_t> g_dust_calls{0}, g_dust_us{0}, g_dust_jobs{0}, g_dust_host{0};
static std::atomic<int> g_dust_high{0};
// WM_SDUST_REPORT=1: the account on stderr when the library is unloaded (a command-line front end has no other way to ask)
static struct DustReport {
	~DustReport()
	{
		if (!getenv("WM_SDUST_REPORT") || !g_dust_calls.load()) return;
		const double calls = (double)g_dust_calls.load(), ms = (double)g_dust_us.load() * 1e-3;
		fprintf(stderr, "[wm] sdust: %.0f window calls, dust kernel %.3f ms in all = %.4f ms per call, %.0f jobs, %.0f finished by the host, largest list %d\n",
		        calls, ms, ms / calls, (double)g_dust_jobs.load(), (double)g_dust_host.load(), g_dust_high.load());
	}
} g_dust_report;
static void dust_note_high(int h) { int cur = g_dust_high.load(); while (h > cur && !g_dust_high.compare_exchange_weak(cur, h)) {} }

// job j: intervals of its sequence -> iv_pool[2 * out_off ..), at most cap pairs; iv_cnt[j] = how many, -1 = finish it on the host; high[j] = largest list held
__global__ __launch_bounds__(64) void sdust_kernel(const wm_sketch_job_t *__restrict__ jobs, const uint8_t *seqs, const uint64_t *rpk, const uint64_t *rnm, int T, int p_cap,
                                                    int *iv_pool, int *iv_cnt, int *high)
{
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int j = blockIdx.x;
	const wm_sketch_job_t s = jobs[j];
	int hi = 0;
	const int n = wmk::sdust_wave(seqs, rpk, rnm, (long long)s.seq_off, s.len, T, (int*)smem, p_cap, iv_pool + 2 * s.out_off, s.cap, &hi);
	if (threadIdx.x == 0) { iv_cnt[j] = n; high[j] = hi; }
}
// the window call's step between the sketch and the seeding: job j's minimizers mini[out_off .. + mcnt[j]) are squeezed in place and mcnt[j] rewritten.
// The intervals live in the job's slice of the sketch's order scratch (dead by now: 8 B per base = one interval per base). A job whose minimizer
// slot overflowed is left to the full-size retry. stat[0]: jobs the host must finish, listed from stat[2] on; stat[1]: largest list held.
__global__ __launch_bounds__(64) void win_dust_kernel(const wm_sketch_job_t *__restrict__ sj, const uint8_t *seqs, const uint64_t *rpk, const uint64_t *rnm, int T, int p_cap,
                                                       wm128_t *mini, int *mcnt, double *so, int *stat)
{
	WM_SETPRIO(2);
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int j = blockIdx.x;
	const wm_sketch_job_t s = sj[j];
	const int n_mini = mcnt[j];
	if (s.len <= 0 || n_mini <= 0 || n_mini > s.cap) return;
	int *iv = (int*)(so + s.scratch_off);
	int hi = 0;
	const int n_iv = wmk::sdust_wave(seqs, rpk, rnm, (long long)s.seq_off, s.len, T, (int*)smem, p_cap, iv, s.len, &hi);
	if (threadIdx.x == 0) atomicMax(stat + 1, hi);
	if (n_iv < 0) {
		if (threadIdx.x == 0) stat[2 + atomicAdd(stat, 1)] = j;
		return;
	}
	simt::mem_sync();                                // lane 0 wrote the intervals, every lane reads them
	const int k = wmk::dust_filter_wave(mini + s.out_off, n_mini, iv, n_iv);
	if (threadIdx.x == 0) mcnt[j] = k;
}
// the codes of the listed jobs as bytes, wherever they live (staged bytes or the packed resident reads): out + stride * scratch_off
__global__ __launch_bounds__(64) void dust_codes_kernel(const wm_sketch_job_t *__restrict__ jobs, const int *list, const uint8_t *seqs, const uint64_t *rpk, const uint64_t *rnm,
                                                         uint8_t *out, int stride)
{
	const wm_sketch_job_t s = jobs[list[blockIdx.x]];
	uint8_t *o = out + (size_t)stride * s.scratch_off;
	for (int i = threadIdx.x; i < s.len; i += 64) o[i] = (uint8_t)wmk::sk_code(seqs, rpk, rnm, (long long)s.seq_off, (long long)i);
}
// the codes of the n_list jobs listed at d_list (host copy: list), fetched to the host
static int dust_fetch_codes(wm_ctx_t *c, const wm_sketch_job_t *h_jobs, const wm_sketch_job_t *d_jobs, const int *list, const int *d_list, int n_list, const uint8_t *d_seqs,
                            uint8_t *d_out, int stride, std::vector<std::vector<uint8_t>> &codes)
{
	hipLaunchKernelGGL(dust_codes_kernel, dim3(n_list), dim3(64), 0, c->stream, d_jobs, d_list, d_seqs, c->d_reads, c->d_reads_nm, d_out, stride);
	HIPCHK(hipGetLastError());
	HIPCHK(ctx_sync(c));
	codes.resize((size_t)n_list);
	for (int q = 0; q < n_list; ++q) {
		const wm_sketch_job_t &s = h_jobs[list[q]];
		codes[q].resize((size_t)s.len + 1);
		HIPCHK(hipMemcpy(codes[q].data(), d_out + (size_t)stride * s.scratch_off, (size_t)s.len, hipMemcpyDeviceToHost));
	}
	return WM_OK;
}

// the filter of a window call (threshold > 0), queued behind the sketch; waits once for the list of jobs the host has to finish (none in practice)
static int window_dust(wm_ctx_t *c, int n, const wm_sketch_job_t *h_sj, const wm_sketch_job_t *d_sj, const uint8_t *d_seqs, int thres, wm128_t *d_mini, int *d_mcnt,
                       double *d_so, uint64_t *d_sx, int *d_stat)
{
	const int p_cap = sdust_list_cap();
	HIPCHK(hipMemsetAsync(d_stat, 0, 8, c->stream));
	HIPCHK(hipEventRecord(c->ev[2], c->stream));
	hipLaunchKernelGGL(win_dust_kernel, dim3(n), dim3(64), (size_t)3 * p_cap * 4, c->stream, d_sj, d_seqs, c->d_reads, c->d_reads_nm, thres, p_cap, d_mini, d_mcnt, d_so, d_stat);
	HIPCHK(hipEventRecord(c->ev[3], c->stream));
	HIPCHK(hipGetLastError());
	int st_pageable[2] = { 0, 0 };
	int *st = c->pin_small ? c->pin_small + 20 : st_pageable;
	HIPCHK(hipMemcpyAsync(st, d_stat, 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));
	float ms = 0; HIPCHK(hipEventElapsedTime(&ms, c->ev[2], c->ev[3]));
	g_dust_calls += 1; g_dust_us += (uint64_t)(ms * 1e3f); g_dust_jobs += (uint64_t)n; g_dust_host += (uint64_t)st[0];
	dust_note_high(st[1]);
	const int n_host = st[0];
	if (n_host <= 0) return WM_OK;
	// the host finishes these jobs (host/wm_sdust.h): their codes and minimizers travel down, the squeezed lists and their sizes back
	std::vector<int> list((size_t)n_host), cnt((size_t)n);
	HIPCHK(hipMemcpy(list.data(), d_stat + 2, (size_t)n_host * 4, hipMemcpyDeviceToHost));
	HIPCHK(hipMemcpy(cnt.data(), d_mcnt, (size_t)n * 4, hipMemcpyDeviceToHost));
	std::vector<std::vector<uint8_t>> codes;
	if (const int rc = dust_fetch_codes(c, h_sj, d_sj, list.data(), d_stat + 2, n_host, d_seqs, (uint8_t*)d_sx, 8, codes)) return rc;
	for (int q = 0; q < n_host; ++q) {
		const int j = list[q];
		const wm_sketch_job_t &s = h_sj[j];
		std::vector<wm::m128> mini((size_t)cnt[j]);
		HIPCHK(hipMemcpy(mini.data(), d_mini + s.out_off, mini.size() * sizeof(wm128_t), hipMemcpyDeviceToHost));
		wm::dust_minimizers(mini, codes[q].data(), s.len, thres);
		const int k = (int)mini.size();
		if (k) HIPCHK(hipMemcpy(d_mini + s.out_off, mini.data(), (size_t)k * sizeof(wm128_t), hipMemcpyHostToDevice));
		HIPCHK(hipMemcpy(d_mcnt + j, &k, 4, hipMemcpyHostToDevice));
	}
	return WM_OK;
}

// ======================================================================================================
// wm_window_batch: sketch → seed → sort → chain fill → chain extraction of n jobs, resident in HBM (window_kernel.h)
// ======================================================================================================
__global__ __launch_bounds__(64) void win_seed_kernel(wm_index_view_t ix, const wm_win_job_t *__restrict__ jobs, const wm_sketch_job_t *__restrict__ sj, const int *__restrict__ mcnt,
                                                       const wm128_t *__restrict__ mini_pool, const wm128_t *__restrict__ pre_pool, int *occ, uint32_t *first, int *emit,
                                                       wm128_t *anchors, uint64_t *used, uint64_t cap, wm_win_res_t *res, int *worst_err)
{
	WM_SETPRIO(2);
	const int j = blockIdx.x;
	const wm_win_job_t jb = jobs[j];
	const wm_sketch_job_t s = sj[j];
	int n_mini = jb.seq_off >= 0 ? mcnt[j] : 0;
	const bool over = n_mini > s.cap;                       // the minimizer slot was too small: the caller retries with full-size slots
	if (over) n_mini = 0;
	wmk::win_seed_wave(ix, jb, mini_pool + s.out_off, n_mini, pre_pool + jb.pre_off, occ + s.out_off, first + s.out_off, emit + s.out_off, anchors, used, cap, res + j);
	if (threadIdx.x == 0) {
		if (over) res[j].err = 1;
		const int e = res[j].err;
		if (e) atomicMax(worst_err, e);
	}
}

// MM_F_HEAP_SORT (launched only by a call that carries the bit, once per size class): the seeded anchors of every job with lo < m <= hi of them go from minimizer
// order into the order of collect_seed_hits_heap (window_kernel.h: heap_order_block) — sorted by the workgroup's stable LSD passes, replayed through the heap when
// two of them share x — and the job is handed on as one whose seeded part needs no sort (win_heap_job). lds_cap > 0: the sort's two buffers and the heap live in LDS
// (2 * lds_cap anchors after the workspace); 0: in buf0 / buf1 and gheap. herr: a word of its own (3 = a job's occurrence counts contradict its anchor count)
template <int NWV>
__global__ __launch_bounds__(64 * NWV) void win_heap_kernel(wm_index_view_t ix, wm_win_job_t *jobs, const wm_sketch_job_t *__restrict__ sj, const wm128_t *__restrict__ mini_pool,
                                                             const int *occ, const uint32_t *first, wm128_t *anchors, wm128_t *buf0, wm128_t *buf1, wm_win_res_t *res, uint64_t *gheap,
                                                             int lo, int hi, int lds_cap, int *herr)
{
	WM_SETPRIO(2);
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	int *lds = (int*)smem;
	wm128_t *stage = (wm128_t*)(lds + WIN_HEAP_INTS(NWV));
	const int j = blockIdx.x;
	const wm_win_res_t r = res[j];
	const wm_sketch_job_t s = sj[j];
	const bool in_lds = lds_cap > 0;
	const int e = wmk::win_heap_job(NWV, ix, jobs + j, r.n_a, r.n_mini, r.err, mini_pool + s.out_off, occ + s.out_off, first + s.out_off, anchors + r.a_off,
	                                in_lds ? stage : buf0 + r.a_off, in_lds ? stage + lds_cap : buf1 + r.a_off, in_lds ? (uint64_t*)stage : (uint64_t*)0, in_lds ? 2 * lds_cap : 0,
	                                gheap + 2 * s.out_off, lo, hi, lds);
	if (e && threadIdx.x == 0) { res[j].err = e; atomicMax(herr, e); }
}

// jobs of at most WIN_SMALL anchors: sorts, fill and extraction by one wavefront in LDS (win_small_wave); larger ones take the kernels below
__global__ __launch_bounds__(64) void win_small_kernel(const wm_win_job_t *__restrict__ jobs, wm_win_res_t *res, const wm128_t *__restrict__ anchors,
                                                        uint64_t *u_pool, wm128_t *v_pool, uint64_t *pool_ctr)
{
	WM_SETPRIO(2);
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	const int j = blockIdx.x;
	const wm_win_res_t r = res[j];
	if (r.n_a <= 0 || r.n_a > wmk::WIN_SMALL || r.err) return;
	wmk::win_small_wave(jobs[j], r.n_a, anchors + r.a_off, smem, res + j, u_pool, v_pool, pool_ctr);
}

// radix_sort_128x of the seeded anchors (src/map.c:252), of the union with the handed-in ones (src/map.c:833), then avg_qspan + the fill's class.
// lds_cap = anchors that fit the dynamic LDS of this launch; a job runs in the launch whose range (lo, lds_cap] holds its size, the last launch
// (lds_cap = 0) takes the rest in global memory
__global__ __launch_bounds__(64) void win_sort_kernel(const wm_win_job_t *__restrict__ jobs, const wm_win_res_t *res, wm128_t *anchors, wm_chain_job_t *cj,
                                                       int *lists, int *counts, int n_jobs, int lo, int lds_cap)
{
	WM_SETPRIO(2);
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	int *ws = (int*)smem;
	wm128_t *stage = (wm128_t*)(ws + ((wmk::WIN_WS_INTS + 3) & ~3));
	const int j = blockIdx.x;
	const wm_win_res_t r = res[j];
	const int n = r.n_a;
	if (n <= lo || (lds_cap > 0 && n > lds_cap) || r.err) return;
	const wm_win_job_t jb = jobs[j];
	wm128_t *a = anchors + r.a_off;
	const bool seeded = jb.seq_off >= 0;
	const int n_pre = jb.n_pre < n ? jb.n_pre : n;
	if (lds_cap > 0) {
		uint64_t *ga = (uint64_t*)a, *la = (uint64_t*)stage;
		if (seeded) {
			for (int i = threadIdx.x; i < 2 * n; i += 64) la[i] = ga[i];
			simt::lds_sync();
			wmk::win_sort_wave<false>(stage + n_pre, n - n_pre, ws);
			if (n_pre > 0) wmk::win_sort_wave<false>(stage, n, ws);
			simt::lds_sync();
			for (int i = threadIdx.x; i < 2 * n; i += 64) ga[i] = la[i];
			wmk::win_plan_wave(jb, j, r.a_off, n, stage, cj, lists, counts, n_jobs);
		} else wmk::win_plan_wave(jb, j, r.a_off, n, a, cj, lists, counts, n_jobs);
	} else {
		if (seeded) {
			wmk::win_sort_wave<true>(a + n_pre, n - n_pre, ws);
			if (n_pre > 0) wmk::win_sort_wave<true>(a, n, ws);
			wmk::win_fence();
		}
		wmk::win_plan_wave(jb, j, r.a_off, n, a, cj, lists, counts, n_jobs);
	}
}

// anchor sets beyond the LDS classes: a whole workgroup sorts (win_bigsort_block: stable, exact whenever the keys are distinct); if two keys tie the
// job falls back to the literal replay of the reference's permutation by one wavefront (win_sort_wave<true>) on the untouched input
// tie_list != 0 (round 5): a job whose keys tie is not replayed here — one lane walking the permutation through global memory costs ~1.5 us per anchor and
// digit level (14 s for the 10^6 anchors of a 5-Mb contig's stage-2 pass, profiles/r05_config5.txt) — but handed to the HOST, where the same serial
// algorithm runs a thousand times faster (window_launch: the ranges of the listed jobs travel down, are sorted by host/wm_core.cpp's radix_sort_128x,
// travel back, and win_plan_list_kernel finishes the job). Entry i of the list (8 ints from tie_list + 8 + 8 i): job, round, a_off lo / hi, n, n_pre.
template <int NWV>
__global__ __launch_bounds__(64 * NWV) void win_bigsort_kernel(const wm_win_job_t *__restrict__ jobs, const wm_win_res_t *res, wm128_t *anchors, wm128_t *buf0, wm128_t *buf1,
                                                               wm_chain_job_t *cj, int *lists, int *counts, int n_jobs, int lo, int *tie_list)
{
	WM_SETPRIO(2);
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	int *big = (int*)smem, *ws = big + ((WIN_BIG_INTS(NWV) + 3) & ~3);
	const int j = blockIdx.x;
	const wm_win_res_t r = res[j];
	const int n = r.n_a;
	if (n <= lo || r.err) return;
	const wm_win_job_t jb = jobs[j];
	wm128_t *a = anchors + r.a_off;
	const int wv = simt::wave_in_block();
	if (jb.seq_off >= 0) {
		const int n_pre = jb.n_pre < n ? jb.n_pre : n;
		for (int round = 0; round < (n_pre > 0 ? 2 : 1); ++round) {           // the seeded anchors (src/map.c:252), then the union with the handed-in ones (:833)
			wm128_t *rng = round == 0 ? a + n_pre : a;
			const int m = round == 0 ? n - n_pre : n;
			int tie = 0;
			const int cur = wmk::win_bigsort_block(NWV, rng, buf0 + r.a_off, buf1 + r.a_off, m, big, &tie);
			if (tie && tie_list) {                 // (uniform over the workgroup) the host finishes this job: this round and what follows it
				if (threadIdx.x == 0) {
					int *e = tie_list + 8 + 8 * atomicAdd(tie_list, 1);
					e[0] = j; e[1] = round; e[2] = (int)(uint32_t)((uint64_t)r.a_off & 0xffffffffu); e[3] = (int)(uint32_t)((uint64_t)r.a_off >> 32); e[4] = n; e[5] = n_pre;
				}
				return;
			}
			if (tie) { if (wv == 0) wmk::win_sort_wave<true>(rng, m, ws); }
			else if (cur >= 0) {
				const uint64_t *src = (const uint64_t*)((cur ? buf1 : buf0) + r.a_off);
				uint64_t *dst = (uint64_t*)rng;
				for (long long i = threadIdx.x; i < 2LL * m; i += 64 * NWV) dst[i] = src[i];
			}
			wmk::win_fence();
			__syncthreads();
		}
	}
	if (wv == 0) wmk::win_plan_wave(jb, j, r.a_off, n, a, cj, lists, counts, n_jobs);
}

// the jobs the host sorted (win_bigsort_kernel's tie list): their fill is planned here
__global__ __launch_bounds__(64) void win_plan_list_kernel(const wm_win_job_t *__restrict__ jobs, const wm_win_res_t *res, const wm128_t *anchors, wm_chain_job_t *cj, int *lists, int *counts,
                                                           int n_jobs, const int *tie_list)
{
	if ((int)blockIdx.x >= tie_list[0]) return;
	const int j = tie_list[8 + 8 * blockIdx.x];
	const wm_win_res_t r = res[j];
	wmk::win_plan_wave(jobs[j], j, r.a_off, r.n_a, anchors + r.a_off, cj, lists, counts, n_jobs);
}

// src/chain.c:89-165 per job; f, p staged in LDS when the job fits (lo, lds_cap], global slab otherwise (lds_cap = 0)
__global__ __launch_bounds__(64) void win_extract_kernel(const wm_win_job_t *__restrict__ jobs, wm_win_res_t *res, wm128_t *anchors, int *fpvt, uint64_t *zu, wm128_t *bbuf, wm128_t *wbuf,
                                                          int lo, int lds_cap, uint64_t *u_pool, wm128_t *v_pool, uint64_t *pool_ctr)
{
	WM_SETPRIO(2);
	extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
	int *ws = (int*)smem;
	const int j = blockIdx.x;
	const wm_win_res_t r = res[j];
	const int n = r.n_a;
	if (n <= lo || (lds_cap > 0 && n > lds_cap) || r.err) return;
	const wm_win_job_t jb = jobs[j];
	int *gf = fpvt + r.a_off * 4, *gp = gf + n, *gv = gp + n, *gt = gv + n;
	if (lds_cap > 0) {
		int *lf = ws + ((wmk::WIN_WS_INTS + 3) & ~3), *lp = lf + lds_cap, *lv = lp + lds_cap, *lt = lv + lds_cap;
		for (int i = threadIdx.x; i < n; i += 64) { lf[i] = gf[i]; lp[i] = gp[i]; }
		simt::lds_sync();
		wmk::win_extract_wave<false>(n, jb.min_cnt, jb.min_sc, anchors + r.a_off, lf, lp, lv, lt, zu + r.a_off, bbuf + r.a_off, wbuf + r.a_off, ws, res + j, u_pool, v_pool, pool_ctr);
	} else
		wmk::win_extract_wave<true>(n, jb.min_cnt, jb.min_sc, anchors + r.a_off, gf, gp, gv, gt, zu + r.a_off, bbuf + r.a_off, wbuf + r.a_off, ws, res + j, u_pool, v_pool, pool_ctr);
}

// what a launched call leaves for its verdict and fetch: the result table and the dense pools on the device, the counters (ctr; tot = chains, anchors, worst err)
struct WinDev { wm_win_res_t *d_res; uint64_t *d_upool; wm128_t *d_vpool; uint64_t *d_ctr; uint64_t ctr[4]; uint32_t tot[3]; };
// device side of one call: everything up to the dense result pools; the caller copies them out. slot_full: full-size minimizer slots (retry)
static int window_launch(wm_ctx_t *c, int n, const wm_window_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes, const wm128_t *pre, size_t n_pre_total,
                         int max_occ, int64_t flag, bool slot_full, WinDev &D, const wm_qkey_t *keys, int sdust_thres)
{
	// host tables
	UBuf<wm_win_job_t> jb(n, c);
	UBuf<wm_sketch_job_t> sj(n, c);
	UBuf<int> ord(n, c);
	uint64_t slots = 0, mtot = 0, stage_hi = 0, pre_hi = 0;
	int bad = -1;
	for (int i = 0; i < n; ++i) {
		const wm_window_job_t &s = jobs[i];
		wm_win_job_t &d = jb[i];
		const bool has_seq = s.seq_off >= -1 && s.len > 0;
		if (s.len < 0 || s.n_pre < 0 || (s.n_pre > 0 && s.pre_off + (uint64_t)s.n_pre > n_pre_total) || s.seq_off < -2 ||
		    (s.seq_off >= 0 && (!c->d_reads || (uint64_t)s.seq_off + (uint64_t)s.len > c->reads_bytes)) ||
		    (s.seq_off == -1 && s.stage_off + (uint64_t)s.len > seqs_bytes)) { if (bad < 0) bad = i; }
		d.seq_off = has_seq ? 0 : -1; d.pre_off = s.pre_off; d.len = s.len; d.n_pre = s.n_pre; d.max_occ = max_occ;
		// (the name bits travel only with a key: skip_seed with qname == NULL ignores them, src/map.c:135)
		d.seed_flag = (int32_t)(flag & (0x100000 | 0x200000 | 0x400000 | (keys && c->d_name_rank ? 3 : 0))); d.q_lo = keys ? keys[i].lo : 0; d.q_eq = keys ? (int32_t)keys[i].eq : 0;
		chain_par_to_job(s.par, d);
		d.min_cnt = s.par.min_cnt; d.min_sc = s.par.min_sc;
		wm_sketch_job_t &k = sj[i];
		k.len = has_seq ? s.len : 0;
		k.cap = has_seq ? (slot_full ? s.len + 1 : s.len / 8 + 16) : 0;
		k.out_off = mtot; mtot += (uint64_t)k.cap;
		k.scratch_off = slots; slots += (uint64_t)k.len;
		k.seq_off = 0;
		if (s.seq_off == -1 && has_seq) stage_hi = std::max<uint64_t>(stage_hi, s.stage_off + (uint64_t)s.len);
		if (s.n_pre > 0) pre_hi = std::max<uint64_t>(pre_hi, s.pre_off + (uint64_t)s.n_pre);
		ord[i] = i;
	}
	if (bad >= 0) return set_err(WM_EINVAL, "window job %d: sequence / anchors outside their buffers (or wm_reads_upload missing)", bad);
	if (c->skp.k < 2) return set_err(WM_EINVAL, "wm_window_batch needs k >= 2 (got %d)", c->skp.k);
	std::sort(ord.begin(), ord.end(), [&](int x, int y) { return sj[x].len != sj[y].len ? sj[x].len > sj[y].len : x < y; });     // sketch: longest first
	// device buffers
	wm_win_job_t *d_jobs = (wm_win_job_t*)arena_take(c, (size_t)n * sizeof(wm_win_job_t));
	wm_sketch_job_t *d_sj = (wm_sketch_job_t*)arena_take(c, (size_t)n * sizeof(wm_sketch_job_t));
	int *d_ord = (int*)arena_take(c, (size_t)n * 4 + 64);
	uint8_t *d_seqs = (uint8_t*)arena_take(c, stage_hi + 64);
	wm128_t *d_pre = (wm128_t*)arena_take(c, (pre_hi + 1) * sizeof(wm128_t));
	double *d_so = (double*)arena_take(c, (slots + 1) * 8);
	uint64_t *d_sx = (uint64_t*)arena_take(c, (slots + 1) * 8);
	uint32_t *d_sy = (uint32_t*)arena_take(c, (slots + 1) * 4), *d_sl = (uint32_t*)arena_take(c, (slots + 1) * 4);
	wm128_t *d_mini = (wm128_t*)arena_take(c, (mtot + 1) * sizeof(wm128_t));
	int *d_mcnt = (int*)arena_take(c, (size_t)n * 4 + 64);
	int *d_occ = (int*)arena_take(c, (mtot + 1) * 4), *d_emit = (int*)arena_take(c, (mtot + 1) * 4);
	uint32_t *d_first = (uint32_t*)arena_take(c, (mtot + 1) * 4);
	D.d_res = (wm_win_res_t*)arena_take(c, (size_t)n * sizeof(wm_win_res_t) + 64);
	wm_chain_job_t *d_cj = (wm_chain_job_t*)arena_take(c, (size_t)n * sizeof(wm_chain_job_t) + 64);
	int *d_lists = (int*)arena_take(c, (size_t)n * 4 * 4 + 64);
	static const bool ties_on_host = !(getenv("WM_WINDOW_TIES_HOST") && atoi(getenv("WM_WINDOW_TIES_HOST")) == 0);      // (0: the literal replay on the device, as until round 4; A/B)
	int *d_tie = ties_on_host ? (int*)arena_take(c, (size_t)(8 + 8 * (size_t)n) * 4) : 0;
	if (ties_on_host && !d_tie) return set_err(WM_ENOMEM, "window batch does not fit the arena");
	int *d_dstat = sdust_thres > 0 ? (int*)arena_take(c, (size_t)(2 + (size_t)n) * 4 + 64) : 0;      // -T: win_dust_kernel's counters and list
	if (sdust_thres > 0 && !d_dstat) return set_err(WM_ENOMEM, "window batch does not fit the arena");
	const bool heap = (flag & wm::F_HEAP_SORT) != 0;                      // --heap-sort=yes: one more scratch array (the heaps that do not fit LDS) and win_heap_kernel, only then
	uint64_t *d_heap = heap ? (uint64_t*)arena_take(c, (mtot + 1) * 16) : 0;
	if (heap && !d_heap) return set_err(WM_ENOMEM, "window batch does not fit the arena");
	uint64_t *d_ctr = (uint64_t*)arena_take(c, 64);          // [0] anchors used, [1] chains in the result pool, [2] anchors in the result pool, [3] worst err (int; the int above it: the heap order's own error, MM_F_HEAP_SORT), [4..5] the four class counts (ints)
	if (!d_jobs || !d_sj || !d_ord || !d_seqs || !d_pre || !d_so || !d_sx || !d_sy || !d_sl || !d_mini || !d_mcnt || !d_occ || !d_emit || !d_first || !D.d_res || !d_cj || !d_lists || !d_ctr)
		return set_err(WM_ENOMEM, "window batch does not fit the arena");
	int *d_counts = (int*)(d_ctr + 4);
	D.d_ctr = d_ctr;
	const size_t long_bytes = sketch_long_bytes(n, sj.data(), !slot_full, c->skp.hpc != 0, !(c->skp.k & 1));       // chunked sketch of long sequences: its tables come before the pool takes the rest
	uint8_t *d_long = long_bytes ? (uint8_t*)arena_take(c, long_bytes) : 0;
	if (long_bytes && !d_long) return set_err(WM_ENOMEM, "window batch does not fit the arena");
	// the rest of the arena is the anchor pool: 72 B per anchor (anchors 16, f|p|v|t 16, z/u 8, b 16, w 16) + the two dense result pools (24)
	const size_t left = c->arena_bytes - ((c->arena_used + 255) & ~(size_t)255);
	const uint64_t cap = left > 4096 ? (left - 4096) / 96 : 0;
	wm128_t *d_a = (wm128_t*)arena_take(c, (cap + 1) * 16);
	int *d_fpvt = (int*)arena_take(c, (cap + 1) * 16);
	uint64_t *d_zu = (uint64_t*)arena_take(c, (cap + 1) * 8);
	wm128_t *d_b = (wm128_t*)arena_take(c, (cap + 1) * 16), *d_w = (wm128_t*)arena_take(c, (cap + 1) * 16);
	D.d_upool = (uint64_t*)arena_take(c, (cap + 1) * 8);
	D.d_vpool = (wm128_t*)arena_take(c, (cap + 1) * 16);
	if (cap < 1024 || !d_a || !d_fpvt || !d_zu || !d_b || !d_w || !D.d_upool || !D.d_vpool) return set_err(WM_ENOMEM, "window batch does not fit the arena");
	if (cap >= ((uint64_t)1 << 31)) return set_err(WM_EINTERNAL, "anchor pool beyond 2^31 entries");      // (32-bit offsets in the result table)
	HIPCHK(hipMemcpyAsync(d_jobs, jb.data(), (size_t)n * sizeof(wm_win_job_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_ord, ord.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
	if (stage_hi) HIPCHK(hipMemcpyAsync(d_seqs, seqs, stage_hi, hipMemcpyHostToDevice, c->stream));
	if (pre_hi) HIPCHK(hipMemcpyAsync(d_pre, pre, pre_hi * sizeof(wm128_t), hipMemcpyHostToDevice, c->stream));
	// staged sequences: byte offsets into d_seqs; resident ones: base indices into the packed reads, flagged (reads2bit.h)
	for (int i = 0; i < n; ++i) if (sj[i].len > 0) sj[i].seq_off = jobs[i].seq_off >= 0 ? (WM_RD_PACKED_BIT | (uint64_t)jobs[i].seq_off) : jobs[i].stage_off;
	HIPCHK(hipMemcpyAsync(d_sj, sj.data(), (size_t)n * sizeof(wm_sketch_job_t), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemsetAsync(D.d_res, 0, (size_t)n * sizeof(wm_win_res_t), c->stream));
	HIPCHK(hipMemsetAsync(d_ctr, 0, 64, c->stream));
	if (d_tie) HIPCHK(hipMemsetAsync(d_tie, 0, 32, c->stream));
	HIPCHK(hipEventRecord(c->ev[0], c->stream));
	if (const int rc = sketch_launch(c, n, sj.data(), d_sj, d_ord, d_seqs, d_so, d_sx, d_sy, d_sl, d_mini, d_mcnt, !slot_full, d_long, long_bytes)) return rc;
	// -T (mm_dust_minier in collect_minimizers, src/map.c:80-81): the minimizers are squeezed before the seeding sees them — n_mini, rep_len and all that follows
	if (sdust_thres > 0) if (const int rc = window_dust(c, n, sj.data(), d_sj, d_seqs, sdust_thres, d_mini, d_mcnt, d_so, d_sx, d_dstat)) return rc;
	wm_index_view_t ix = { c->d_hkey, c->d_hval, c->d_P, c->hbits, 0, c->d_name_rank, c->d_seq_len };
	hipLaunchKernelGGL(win_seed_kernel, dim3(n), dim3(64), 0, c->stream, ix, d_jobs, d_sj, d_mcnt, d_mini, d_pre, d_occ, d_first, d_emit, d_a, d_ctr, cap, D.d_res, (int*)(d_ctr + 3));
	const size_t ws_bytes = (size_t)wmk::WIN_WS_PAD * 4;
	constexpr int kSmall = wmk::WIN_SMALL, kLarge = wmk::WIN_LARGE;
	if (heap) {      // three size classes of the seeded part, LDS sized per class (window_kernel.h: heap_order_launch)
		int *d_herr = (int*)(d_ctr + 3) + 1;
		if (const int rc = wmk::heap_order_launch([&](auto nwv, size_t lds, int lo, int hi, int lds_cap) -> int {
			constexpr int N = decltype(nwv)::value;
			HIPCHK(hipFuncSetAttribute((const void*)win_heap_kernel<N>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
			hipLaunchKernelGGL(win_heap_kernel<N>, dim3(n), dim3(64 * N), lds, c->stream, ix, d_jobs, d_sj, d_mini, d_occ, d_first, d_a, d_b, d_w, D.d_res, d_heap, lo, hi, lds_cap, d_herr);
			return WM_OK;
		})) return rc;
	}
	// the bulk (jobs of at most WIN_SMALL anchors: one MCAS window yields ~100) finishes in one kernel; the rest goes class by class
	HIPCHK(hipFuncSetAttribute((const void*)win_small_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
	hipLaunchKernelGGL(win_small_kernel, dim3(n), dim3(64), (size_t)wmk::WIN_SMALL_LDS, c->stream, d_jobs, D.d_res, d_a, D.d_upool, D.d_vpool, d_ctr + 1);
	HIPCHK(hipFuncSetAttribute((const void*)win_sort_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
	hipLaunchKernelGGL(win_sort_kernel, dim3(n), dim3(64), ws_bytes + (size_t)kLarge * 16, c->stream, d_jobs, D.d_res, d_a, d_cj, d_lists, d_counts, n, kSmall, kLarge);
	{
		constexpr int NWV = 8;
		const size_t big_bytes = (size_t)((WIN_BIG_INTS(NWV) + 3) & ~3) * 4 + ws_bytes;
		hipLaunchKernelGGL(win_bigsort_kernel<NWV>, dim3(n), dim3(64 * NWV), big_bytes, c->stream, d_jobs, D.d_res, d_a, d_b, d_w, d_cj, d_lists, d_counts, n, kLarge, d_tie);
	}
	if (d_tie) {
		// large anchor sets whose keys tie: the exact order of equal keys is the reference's unstable sort's (src/ksort.h:101-151), a serial algorithm —
		// serial work belongs on the host. One small read-back per window call; the ranges travel only when there are such jobs.
		int *h_cnt = c->pin_small ? c->pin_small + 16 : 0;
		int cnt_pageable = 0;
		HIPCHK(hipMemcpyAsync(h_cnt ? h_cnt : &cnt_pageable, d_tie, 4, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(ctx_sync(c));
		const int n_tie = h_cnt ? *h_cnt : cnt_pageable;
		if (n_tie > 0) {
			UBuf<int> tl((size_t)8 * n_tie, c);
			HIPCHK(hipMemcpyAsync(tl.data(), d_tie + 8, (size_t)8 * n_tie * 4, hipMemcpyDeviceToHost, c->stream));
			HIPCHK(ctx_sync(c));
			std::vector<uint64_t> off((size_t)n_tie + 1, 0);
			for (int i = 0; i < n_tie; ++i) off[i + 1] = off[i] + (uint64_t)tl[8 * i + 4];
			UBuf<wm128_t> ha((size_t)off[n_tie] + 1, c);
			for (int i = 0; i < n_tie; ++i) {
				const uint64_t a_off = (uint64_t)(uint32_t)tl[8 * i + 2] | (uint64_t)(uint32_t)tl[8 * i + 3] << 32;
				HIPCHK(hipMemcpyAsync(ha.data() + off[i], d_a + a_off, (size_t)tl[8 * i + 4] * 16, hipMemcpyDeviceToHost, c->stream));
			}
			HIPCHK(ctx_sync(c));
			{
				WM_SITE("window.tie_sort");
				wm::parallel_for(c->host_threads, (size_t)n_tie, [&](size_t i) {
					wm::m128 *a0 = (wm::m128*)(ha.data() + off[i]);
					const int nn = tl[8 * i + 4], round = tl[8 * i + 1], n_pre = std::min(tl[8 * i + 5], nn);
					if (round == 0) wm::radix_sort_128x(a0 + n_pre, a0 + nn);                    // the seeded anchors (src/map.c:252) ...
					if (round == 1 || n_pre > 0) wm::radix_sort_128x(a0, a0 + nn);               // ... then the union with the handed-in ones (:833)
				});
			}
			for (int i = 0; i < n_tie; ++i) {
				const uint64_t a_off = (uint64_t)(uint32_t)tl[8 * i + 2] | (uint64_t)(uint32_t)tl[8 * i + 3] << 32;
				HIPCHK(hipMemcpyAsync(d_a + a_off, ha.data() + off[i], (size_t)tl[8 * i + 4] * 16, hipMemcpyHostToDevice, c->stream));
			}
			hipLaunchKernelGGL(win_plan_list_kernel, dim3(n_tie), dim3(64), 0, c->stream, d_jobs, D.d_res, d_a, d_cj, d_lists, d_counts, n, d_tie);
			HIPCHK(ctx_sync(c));                 // (the staging buffers above are released at the end of this block)
		}
	}
	{   // the fill, per class list (chain_fill.h). The dense fill is 16 x 5 — a whole max_iter window per step — or, with WM_CHAIN_WIDE=0, the round-5 one; the
		// switches are read once per process. Class 3, at most WIN_SMALL anchors, was served by win_small_kernel
		static const ChainDense dense = chain_dense_env(false);
		const ChainFillList cls[4] = { { d_lists, d_counts, n }, { d_lists + n, d_counts + 1, n }, { d_lists + 2 * (size_t)n, d_counts + 2, n }, { 0, 0, 0 } };
		if (const int rc = chain_fill_launch(c->stream, d_cj, d_a, d_fpvt, cls, dense)) return rc;
	}
	HIPCHK(hipFuncSetAttribute((const void*)win_extract_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
	hipLaunchKernelGGL(win_extract_kernel, dim3(n), dim3(64), ws_bytes + (size_t)kLarge * 16, c->stream, d_jobs, D.d_res, d_a, d_fpvt, d_zu, d_b, d_w, kSmall, kLarge, D.d_upool, D.d_vpool, d_ctr + 1);
	hipLaunchKernelGGL(win_extract_kernel, dim3(n), dim3(64), ws_bytes, c->stream, d_jobs, D.d_res, d_a, d_fpvt, d_zu, d_b, d_w, kLarge, 0, D.d_upool, D.d_vpool, d_ctr + 1);
	HIPCHK(hipEventRecord(c->ev[1], c->stream));
	HIPCHK(hipGetLastError());
	uint64_t *h_ctr = c->pin_small ? (uint64_t*)(c->pin_small + 8) : D.ctr;
	HIPCHK(hipMemcpyAsync(h_ctr, d_ctr, 32, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));                  // (also: the host tables above are read by the copies until here)
	memcpy(D.ctr, h_ctr, 32);
	D.tot[0] = (uint32_t)D.ctr[1]; D.tot[1] = (uint32_t)D.ctr[2]; D.tot[2] = (uint32_t)(D.ctr[3] & 0xffffffffu);
	float ms = 0; HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); c->aux_ms += ms;
	return WM_OK;
}

// copies the result table and the two dense pools of a launched call to the host (pools sized by the caller from D.tot)
static int window_fetch(wm_ctx_t *c, const WinDev &D, int n, wm_window_res_t *res, uint64_t *u_pool, wm128_t *a_pool)
{
	UBuf<wm_win_res_t> hr(n, c);
	HIPCHK(hipMemcpyAsync(hr.data(), D.d_res, (size_t)n * sizeof(wm_win_res_t), hipMemcpyDeviceToHost, c->stream));
	if (D.tot[0]) HIPCHK(hipMemcpyAsync(u_pool, D.d_upool, (size_t)D.tot[0] * 8, hipMemcpyDeviceToHost, c->stream));
	if (D.tot[1]) HIPCHK(hipMemcpyAsync(a_pool, D.d_vpool, (size_t)D.tot[1] * 16, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));
	for (int i = 0; i < n; ++i) {
		const wm_win_res_t &r = hr[i];
		res[i].n_anchors = r.n_a; res[i].rep_len = r.rep_len; res[i].n_mini = r.n_mini; res[i].n_u = r.n_u; res[i].n_v = r.n_v; res[i].u_off = r.u_out; res[i].a_off = r.v_out;
	}
	return WM_OK;
}
// verdict of a launched call: 0 = fetch, 1 = launch again with full-size minimizer slots, < 0 = error
static int window_verdict(const WinDev &D, int round)
{
	if (D.tot[2] == 2) return set_err(WM_ENOMEM, "window batch does not fit the arena (anchor pool)");
	if (D.ctr[3] >> 32) return set_err(WM_EINTERNAL, "heap-ordered seeding: a job's occurrence counts contradict its anchor count");
	if (D.tot[2] == 1) return round == 0 ? 1 : set_err(WM_EINTERNAL, "minimizer slot overflow at full size");
	return 0;
}

// one window call, shared by wm_window_batch* and the mapper (wm_rt.h): two rounds at most, the second with full-size minimizer slots
int window_run(wm_ctx_t *c, int n, const wm_window_job_t *jobs, const wm_qkey_t *keys, const uint8_t *seqs, size_t seqs_bytes, const wm128_t *pre, size_t n_pre_total,
               int max_occ, int64_t flag, int sdust_thres, wm_window_res_t *res, const WinSized &sized)
{
	c->aux_ms = 0;
	for (int round = 0; round < 2; ++round) {
		ArenaMark mark(c);
		WinDev D;
		int rc = window_launch(c, n, jobs, seqs, seqs_bytes, pre, n_pre_total, max_occ, flag, round == 1, D, keys, sdust_thres);
		if (rc) return rc;
		rc = window_verdict(D, round);
		if (rc < 0) return rc;
		if (rc == 1) continue;
		uint64_t *u_pool = 0;
		wm128_t *a_pool = 0;
		if ((rc = sized(D.tot[0], D.tot[1], &u_pool, &a_pool)) != 0) return rc;
		return window_fetch(c, D, n, res, u_pool, a_pool);
	}
	return set_err(WM_EINTERNAL, "window retry did not converge");
}

extern "C" int wm_window_batch(wm_ctx_t *c, int n, const wm_window_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes, const wm128_t *pre, size_t n_pre_total,
                               int max_occ, int64_t flag, wm_window_res_t *res, uint64_t *u_pool, size_t u_cap, size_t *u_used, wm128_t *a_pool, size_t a_cap, size_t *a_used)
{
	return wm_window_batch_keyed(c, n, jobs, 0, seqs, seqs_bytes, pre, n_pre_total, max_occ, flag, res, u_pool, u_cap, u_used, a_pool, a_cap, a_used);
}

extern "C" int wm_window_batch_keyed(wm_ctx_t *c, int n, const wm_window_job_t *jobs, const wm_qkey_t *keys, const uint8_t *seqs, size_t seqs_bytes, const wm128_t *pre, size_t n_pre_total,
                                     int max_occ, int64_t flag, wm_window_res_t *res, uint64_t *u_pool, size_t u_cap, size_t *u_used, wm128_t *a_pool, size_t a_cap, size_t *a_used)
{
	return wm_window_batch_dust(c, n, jobs, keys, seqs, seqs_bytes, pre, n_pre_total, max_occ, flag, 0, res, u_pool, u_cap, u_used, a_pool, a_cap, a_used);
}

extern "C" int wm_window_batch_dust(wm_ctx_t *c, int n, const wm_window_job_t *jobs, const wm_qkey_t *keys, const uint8_t *seqs, size_t seqs_bytes, const wm128_t *pre, size_t n_pre_total,
                                    int max_occ, int64_t flag, int sdust_thres, wm_window_res_t *res, uint64_t *u_pool, size_t u_cap, size_t *u_used, wm128_t *a_pool, size_t a_cap, size_t *a_used)
try {
	if (u_used) *u_used = 0;
	if (a_used) *a_used = 0;
	if (!c || !c->have_index) return set_err(WM_EINVAL, "wm_index_upload has not been called on this context");
	if (n <= 0) return WM_OK;
	if (!jobs || !res) return set_err(WM_EINVAL, "null argument");
	HIPCHK(hipSetDevice(c->device));
	return window_run(c, n, jobs, keys, seqs, seqs_bytes, pre, n_pre_total, max_occ, flag, sdust_thres, res, [&](uint32_t n_chains, uint32_t n_anchors, uint64_t **up, wm128_t **ap) {
		if (u_used) *u_used = n_chains;
		if (a_used) *a_used = n_anchors;
		if (n_chains > u_cap || n_anchors > a_cap) return set_err(WM_ENOMEM, "result pools too small: need %u chains and %u anchors", n_chains, n_anchors);
		if ((n_chains && !u_pool) || (n_anchors && !a_pool)) return set_err(WM_EINVAL, "null result pool");
		*up = u_pool; *ap = a_pool;
		return WM_OK;
	});
}
catch (const std::bad_alloc &) { return set_err(WM_ENOMEM, "out of host memory"); }


// ======================================================================================================
// wm_sdust_batch: the operator on its own
// ======================================================================================================
extern "C" int wm_sdust_batch(wm_ctx_t *c, int n, const uint8_t *seqs, size_t seqs_bytes, const uint64_t *seq_off, const int32_t *len, const uint8_t *resident, int thres,
                              int32_t *iv, size_t iv_cap, uint64_t *iv_off, int32_t *n_iv, int32_t *p_high)
try {
	if (!c) return set_err(WM_EINVAL, "null context");
	if (n <= 0) return WM_OK;
	if (!seq_off || !len || !iv_off || !n_iv || (!seqs && seqs_bytes)) return set_err(WM_EINVAL, "null argument");
	if (thres <= 0) return set_err(WM_EINVAL, "wm_sdust_batch needs a threshold > 0 (got %d)", thres);
	HIPCHK(hipSetDevice(c->device));
	ArenaMark mark(c);
	std::vector<wm_sketch_job_t> jb((size_t)n);
	uint64_t slots = 0, bases = 0;
	for (int i = 0; i < n; ++i) {
		const bool res = resident && resident[i];
		if (len[i] < 0 || (res ? (!c->d_reads || seq_off[i] + (uint64_t)len[i] > c->reads_bytes) : (seq_off[i] + (uint64_t)len[i] > seqs_bytes))) return set_err(WM_EINVAL, "sequence %d outside its buffer", i);
		jb[i].seq_off = res ? (WM_RD_PACKED_BIT | seq_off[i]) : seq_off[i]; jb[i].len = len[i];
		jb[i].cap = len[i] / 4 + 24;                                   // intervals are disjoint, apart and at least three bases long, and end at most a window past the sequence
		jb[i].out_off = slots; slots += (uint64_t)jb[i].cap;
		jb[i].scratch_off = bases; bases += (uint64_t)len[i];
	}
	const int p_cap = sdust_list_cap();
	wm_sketch_job_t *d_jobs = (wm_sketch_job_t*)arena_take(c, (size_t)n * sizeof(wm_sketch_job_t));
	uint8_t *d_seqs = (uint8_t*)arena_take(c, seqs_bytes + 64);
	int *d_iv = (int*)arena_take(c, (size_t)(slots + 1) * 8), *d_cnt = (int*)arena_take(c, (size_t)n * 4 + 64), *d_high = (int*)arena_take(c, (size_t)n * 4 + 64);
	if (!d_jobs || !d_seqs || !d_iv || !d_cnt || !d_high) return set_err(WM_ENOMEM, "sdust batch does not fit the arena");
	HIPCHK(hipMemcpyAsync(d_jobs, jb.data(), (size_t)n * sizeof(wm_sketch_job_t), hipMemcpyHostToDevice, c->stream));
	if (seqs_bytes) HIPCHK(hipMemcpyAsync(d_seqs, seqs, seqs_bytes, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipEventRecord(c->ev[0], c->stream));
	hipLaunchKernelGGL(sdust_kernel, dim3(n), dim3(64), (size_t)3 * p_cap * 4, c->stream, d_jobs, d_seqs, c->d_reads, c->d_reads_nm, thres, p_cap, d_iv, d_cnt, d_high);
	HIPCHK(hipEventRecord(c->ev[1], c->stream));
	HIPCHK(hipGetLastError());
	std::vector<int> cnt((size_t)n), high((size_t)n);
	std::vector<int32_t> tmp((size_t)(slots + 1) * 2);
	HIPCHK(hipMemcpyAsync(cnt.data(), d_cnt, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(high.data(), d_high, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(hipMemcpyAsync(tmp.data(), d_iv, (size_t)slots * 8, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));
	float ms = 0; HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev[1])); c->aux_ms = ms;
	// jobs whose list overflowed: finished by the host restatement
	std::vector<int> list;
	for (int i = 0; i < n; ++i) if (cnt[i] < 0) list.push_back(i);
	std::vector<std::vector<wm::DustIv>> hiv(list.size());
	if (!list.empty()) {
		int *d_list = (int*)arena_take(c, list.size() * 4 + 64);
		uint8_t *d_codes = (uint8_t*)arena_take(c, (size_t)bases + 64);
		if (!d_list || !d_codes) return set_err(WM_ENOMEM, "sdust batch does not fit the arena");
		HIPCHK(hipMemcpy(d_list, list.data(), list.size() * 4, hipMemcpyHostToDevice));
		std::vector<std::vector<uint8_t>> codes;
		if (const int rc = dust_fetch_codes(c, jb.data(), d_jobs, list.data(), d_list, (int)list.size(), d_seqs, d_codes, 1, codes)) return rc;
		for (size_t q = 0; q < list.size(); ++q) high[list[q]] = wm::sdust_intervals(codes[q].data(), len[list[q]], thres, hiv[q]);
		g_dust_host += (uint64_t)list.size();
	}
	size_t used = 0, q = 0;
	for (int i = 0; i < n; ++i) {
		const bool host = cnt[i] < 0;
		const size_t k = host ? hiv[q].size() : (size_t)cnt[i];
		if (used + k > iv_cap || (k && !iv)) return set_err(WM_ENOMEM, "interval output pool too small");
		iv_off[i] = used; n_iv[i] = (int32_t)k;
		if (host) { for (size_t t = 0; t < k; ++t) { iv[2 * (used + t)] = hiv[q][t].st; iv[2 * (used + t) + 1] = hiv[q][t].en; } ++q; }
		else if (k) memcpy(iv + 2 * used, tmp.data() + 2 * jb[i].out_off, k * 8);
		used += k;
		if (p_high) p_high[i] = high[i];
		dust_note_high(high[i]);
	}
	return WM_OK;
}
catch (const std::bad_alloc &) { return set_err(WM_ENOMEM, "out of host memory"); }

extern "C" void wm_sdust_stats(double *out5, int reset)
{
	if (out5) { out5[0] = (double)g_dust_calls.load(); out5[1] = (double)g_dust_us.load() * 1e-3; out5[2] = (double)g_dust_jobs.load(); out5[3] = (double)g_dust_host.load(); out5[4] = (double)g_dust_high.load(); }
	if (reset) { g_dust_calls = 0; g_dust_us = 0; g_dust_jobs = 0; g_dust_host = 0; g_dust_high = 0; }
}

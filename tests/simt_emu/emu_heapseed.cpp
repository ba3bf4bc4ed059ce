// tests/simt_emu/emu_heapseed.cpp — TEST INFRASTRUCTURE ONLY.
// MM_F_HEAP_SORT (--heap-sort=yes) on the host wavefront emulator: the two seeding kernels followed by the ordering stage of their launchers
// (win_heap_job / seed_heap_job of csrc/window_kernel.h — the bodies of the heap kernels —, then the sorts a window job goes through afterwards), with event counters that say which
// road a job took, and the host restatement of collect_seed_hits_heap (csrc/host/wm_core.cpp) — through a C ABI for ctypes.
#include "simt.h"                    // the emulator (this directory is first on the include path)
static long g_hev[4];
#define WM_HEAP_EVENT(k) (++g_hev[k])      // 0: sorted list kept (no equal x), 1: heap replayed, 2: heap in global memory
#include "seedchain_kernel.h"        // winnowmap_amd/csrc
#include "window_kernel.h"
#include "host/wm_core.h"
#include <vector>
#include <thread>

namespace {

struct Head {       // what every entry point takes first
	const uint64_t *hkey, *hval, *P; int hbits; const uint32_t *name_rank, *seq_len; const uint64_t *mx, *my; int n_mini, qlen, max_occ, flag; uint32_t q_lo; int q_eq;
};
#define HEAD_ARGS const uint64_t *hkey, const uint64_t *hval, const uint64_t *P, int hbits, const uint32_t *name_rank, const uint32_t *seq_len, \
                  const uint64_t *mx, const uint64_t *my, int n_mini, int qlen, int max_occ, int flag, uint32_t q_lo, int q_eq
#define HEAD_PACK Head{ hkey, hval, P, hbits, name_rank, seq_len, mx, my, n_mini, qlen, max_occ, flag, q_lo, q_eq }

const int FILT = 0x100000 | 0x200000 | 3;

} // namespace

extern "C" {

void emu_heap_events(long *out, int reset)
{
	for (int i = 0; i < 4; ++i) { out[i] = g_hev[i]; if (reset) g_hev[i] = 0; }
}

// the host's heap primitives on (x, y) pairs
void emu_host_heapmake(size_t n, uint64_t *x, uint64_t *y)
{
	std::vector<wm::m128> l(n + 1);
	for (size_t i = 0; i < n; ++i) l[i].x = x[i], l[i].y = y[i];
	wm::ks_heapmake_heap(n, l.data());
	for (size_t i = 0; i < n; ++i) x[i] = l[i].x, y[i] = l[i].y;
}
void emu_host_heapdown(size_t i0, size_t n, uint64_t *x, uint64_t *y)
{
	std::vector<wm::m128> l(n + 1);
	for (size_t i = 0; i < n; ++i) l[i].x = x[i], l[i].y = y[i];
	wm::ks_heapdown_heap(i0, n, l.data());
	for (size_t i = 0; i < n; ++i) x[i] = l[i].x, y[i] = l[i].y;
}

// collect_matches (src/map.c:97-130) on the flat table, then wm::seed_hits_heap; has_key: the query carries a name key. res_out = n_a, rep_len
int emu_host_seed_heap(HEAD_ARGS, int has_key, uint64_t *ax, uint64_t *ay, int cap, int32_t *res_out)
{
	const uint64_t hmask = ((uint64_t)1 << hbits) - 1;
	std::vector<wm::HeapMatch> m;
	int rep_st = 0, rep_en = 0, rep_len = 0;
	int64_t n_a = 0;
	for (int i = 0; i < n_mini; ++i) {
		const uint64_t key = mx[i] >> 8;
		uint64_t s = (key * 0x9E3779B97F4A7C15ULL) >> (64 - hbits), first = 0;
		int t = 0;
		for (uint64_t guard = 0; guard <= hmask; ++guard, s = (s + 1) & hmask) {
			if (hkey[s] == key) { t = (int)(hval[s] & 0xffffffffu); first = hval[s] >> 32; break; }
			if (hkey[s] == ~(uint64_t)0) break;
		}
		const uint32_t q_pos = (uint32_t)my[i], q_span = (uint32_t)(mx[i] & 0xff);
		if (t >= max_occ) {
			const int en = (int)(q_pos >> 1) + 1, st = en - (int)q_span;
			if (st > rep_en) { rep_len += rep_en - rep_st; rep_st = st; rep_en = en; } else rep_en = en;
		} else {
			wm::HeapMatch q;
			q.n = (uint32_t)t; q.q_pos = q_pos; q.q_span = q_span; q.cr = P + first;
			q.is_tandem = (i > 0 && mx[i - 1] >> 8 == key) || (i < n_mini - 1 && mx[i + 1] >> 8 == key);
			m.push_back(q);
			n_a += t;
		}
	}
	rep_len += rep_en - rep_st;
	std::vector<wm::m128> a((size_t)n_a + 1);
	wm::SeedSkip sk;
	sk.flag = flag; sk.has_key = has_key != 0; sk.q_lo = q_lo; sk.q_eq = q_eq; sk.name_rank = name_rank; sk.seq_len = seq_len;
	const int64_t k = wm::seed_hits_heap(m.data(), (int)m.size(), n_a, qlen, sk, a.data());
	if (k > cap) return -1;
	for (int64_t i = 0; i < k; ++i) ax[i] = a[i].x, ay[i] = a[i].y;
	res_out[0] = (int32_t)k; res_out[1] = rep_len;
	return 0;
}

} // extern "C"

namespace {

// a workgroup of nwv wavefronts (one thread each, a barrier between them) runs body(wavefront)
template <class F> void run_block(int nwv, F body)
{
	pthread_barrier_t bar;
	pthread_barrier_init(&bar, 0, nwv);
	simt::block_barrier() = &bar;
	std::vector<std::thread> th;
	for (int w = 0; w < nwv; ++w) th.emplace_back([&, w]() { simt::wave_slot() = w; simt::exec_mask() = ~0ull; body(w); });
	for (auto &t : th) t.join();
	simt::block_barrier() = 0;
	pthread_barrier_destroy(&bar);
	simt::wave_slot() = 0; simt::exec_mask() = ~0ull;
}

// the launchers' three size classes of the heap kernels (wm_window.hip / wm_index.hip): at most small_cap anchors — one wavefront, buffers and heap in "LDS";
// at most lds_cap — nwv wavefronts, "LDS"; more — nwv wavefronts, global buffers and heap. job(NWV, b0, b1, hl, hcap, lo, hi, lds) is the kernel's body
template <class F> int heap_classes(int small_cap, int lds_cap, int nwv, int n_max, F job)
{
	if (small_cap > lds_cap) small_cap = lds_cap;
	std::vector<wm128_t> stage(2 * (size_t)lds_cap + 2), g0(n_max + 1), g1(n_max + 1);
	const int lo[3] = { -1, small_cap, lds_cap }, hi[3] = { small_cap, lds_cap, 0x7fffffff }, wv[3] = { 1, nwv, nwv };
	int err = 0;
	for (int k = 0; k < 3 && !err; ++k) {
		std::vector<int> lds(WIN_HEAP_INTS(wv[k]) + 8, 0x5a5a5a5a);
		const int cap = k == 0 ? small_cap : lds_cap;
		run_block(wv[k], [&](int w) {
			const int e = k < 2 ? job(wv[k], stage.data(), stage.data() + cap, (uint64_t*)stage.data(), 2 * cap, lo[k], hi[k], lds.data())
			                    : job(wv[k], g0.data(), g1.data(), (uint64_t*)0, 0, lo[k], hi[k], lds.data());
			if (w == 0) err = e;
		});
	}
	return err;
}

} // namespace

extern "C" {

// wm_seed_batch's device side for one job: seed_wave, then — with the heap bit — the seed_heap_kernel launches (seed_heap_job; lds_cap anchors of "LDS", the
// one-wavefront class up to 16); without it the radix replay the host applies. res_out = n_anchors, rep_len; returns the heap order's verdict
int emu_heap_seed(HEAD_ARGS, int lds_cap, uint64_t *ax, uint64_t *ay, int cap, int32_t *res_out)
{
	const Head h = HEAD_PACK;
	wm_index_view_t ix = { h.hkey, h.hval, h.P, h.hbits, 0, h.name_rank, h.seq_len };
	std::vector<wm128_t> mini(n_mini + 1), anc(cap + 1);
	for (int i = 0; i < n_mini; ++i) mini[i].x = mx[i], mini[i].y = my[i];
	wm_seed_job_t jb;
	memset(&jb, 0, sizeof(jb));
	jb.n_mini = n_mini; jb.qlen = qlen; jb.max_occ = max_occ; jb.cap = cap; jb.flag = flag & FILT; jb.q_lo = q_lo; jb.q_eq = q_eq;
	std::vector<int> occ(n_mini + 1), ws(wmk::WIN_WS_PAD);
	std::vector<uint32_t> first(n_mini + 1);
	std::vector<uint64_t> gheap(2 * (size_t)n_mini + 2);
	wm_seed_res_t res = { 0, 0 };
	simt::exec_mask() = ~0ull;
	const bool heap = (flag & wmk::WM_SEED_HEAP_BIT) != 0;
	wmk::seed_wave(ix, jb, mini.data(), anc.data(), occ.data(), &res, heap ? first.data() : 0);
	res_out[0] = res.n_anchors; res_out[1] = res.rep_len;
	if (res.n_anchors > cap) return -1;
	int e = 0;
	if (heap) e = heap_classes(16, lds_cap, 3, cap, [&](int NWV, wm128_t *b0, wm128_t *b1, uint64_t *hl, int hcap, int lo, int hi, int *lds) {
		return wmk::seed_heap_job(NWV, ix, jb, res.n_anchors, mini.data(), occ.data(), first.data(), anc.data(), b0, b1, hl, hcap, gheap.data(), lo, hi, lds); });
	else wmk::win_sort_wave<true>(anc.data(), res.n_anchors, ws.data());
	for (int i = 0; i < res.n_anchors; ++i) ax[i] = anc[i].x, ay[i] = anc[i].y;
	return e;
}

// a window job up to the list its chain fill reads: win_seed_wave, with the heap bit the win_heap_kernel launches (win_heap_job: orders the seeded part and hands the
// job on, lds_cap anchors of "LDS", the one-wavefront class up to 16), then the ordering of the job's class exactly as a call without the bit runs it, read from the
// job as win_heap_job left it — at most sort_cap anchors: one wavefront (win_small_wave / win_sort_kernel), more: the workgroup of nwv wavefronts (win_bigsort_kernel,
// ties by the radix replay). seeded = 0: a job without a sequence (only handed-in anchors). res_out = n_a, rep_len, err, 1 if the workgroup road was taken
int emu_heap_window(HEAD_ARGS, int seeded, int n_pre, const uint64_t *px, const uint64_t *py, int lds_cap, int sort_cap, int nwv, uint64_t *ax, uint64_t *ay, int cap, int32_t *res_out)
{
	const Head h = HEAD_PACK;
	wm_index_view_t ix = { h.hkey, h.hval, h.P, h.hbits, 0, h.name_rank, h.seq_len };
	std::vector<wm128_t> mini(n_mini + 1), pre(n_pre + 1), pool(cap + 64);
	for (int i = 0; i < n_mini; ++i) mini[i].x = mx[i], mini[i].y = my[i];
	for (int i = 0; i < n_pre; ++i) pre[i].x = px[i], pre[i].y = py[i];
	wm_win_job_t jb;
	memset(&jb, 0, sizeof(jb));
	jb.seq_off = seeded ? 0 : -1; jb.len = qlen; jb.n_pre = n_pre; jb.max_occ = max_occ; jb.seed_flag = flag & (FILT | wmk::WM_SEED_HEAP_BIT); jb.q_lo = q_lo; jb.q_eq = q_eq;
	std::vector<int> occ(n_mini + 1), emit(n_mini + 1), ws(wmk::WIN_WS_PAD);
	std::vector<uint32_t> first(n_mini + 1);
	std::vector<uint64_t> gheap(2 * (size_t)n_mini + 2);
	uint64_t used = 5;
	wm_win_res_t res;
	memset(&res, 0, sizeof(res));
	simt::exec_mask() = ~0ull;
	wmk::win_seed_wave(ix, jb, mini.data(), seeded ? n_mini : 0, pre.data(), occ.data(), first.data(), emit.data(), pool.data(), &used, (uint64_t)cap, &res);
	res_out[0] = res.n_a; res_out[1] = res.rep_len; res_out[2] = res.err; res_out[3] = 0;
	if (res.err) return 0;
	const int n = res.n_a;
	wm128_t *a = pool.data() + res.a_off;
	int err = 0;
	if (jb.seed_flag & wmk::WM_SEED_HEAP_BIT)         // win_heap_kernel, three classes; jb is rewritten
		err = heap_classes(16, lds_cap, nwv, n, [&](int NWV, wm128_t *b0, wm128_t *b1, uint64_t *hl, int hcap, int lo, int hi, int *lds) {
			return wmk::win_heap_job(NWV, ix, &jb, res.n_a, res.n_mini, res.err, mini.data(), occ.data(), first.data(), a, b0, b1, hl, hcap, gheap.data(), lo, hi, lds); });
	// what follows reads the job only, as the class kernels do
	const bool sorted_here = jb.seq_off >= 0;
	const int np = jb.n_pre < n ? jb.n_pre : n, m = n - np;
	if (!err && sorted_here && n > 0 && n <= sort_cap) {   // win_small_wave / win_sort_kernel
		wmk::win_sort_wave<true>(a + np, m, ws.data());
		if (np > 0) wmk::win_sort_wave<true>(a, n, ws.data());
	} else if (!err && sorted_here && n > 0) {              // win_bigsort_kernel
		res_out[3] = 1;
		std::vector<wm128_t> b0(n + 1), b1(n + 1);
		std::vector<int> big(WIN_BIG_INTS(nwv) + 8, 0x5a5a5a5a);
		run_block(nwv, [&](int w) {
			for (int round = 0; round < (np > 0 ? 2 : 1); ++round) {
				wm128_t *rng = round == 0 ? a + np : a;
				const int mm = round == 0 ? m : n;
				int tie = 0;
				const int cur = wmk::win_bigsort_block(nwv, rng, b0.data(), b1.data(), mm, big.data(), &tie);
				if (tie) { if (w == 0) wmk::win_sort_wave<true>(rng, mm, ws.data()); }
				else if (cur >= 0) { if (w == 0) memcpy(rng, cur ? b1.data() : b0.data(), (size_t)mm * sizeof(wm128_t)); }
				simt::block_sync();
			}
		});
	}
	if (err) res_out[2] = err;
	for (int i = 0; i < n; ++i) ax[i] = a[i].x, ay[i] = a[i].y;
	return err;
}

} // extern "C"

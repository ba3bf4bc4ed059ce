// sdust_kernel.h — the reference's -T filter on gfx950: the symmetric-DUST intervals of a sequence (sdust_core, src/sdust.c:134-164, W = 64 as
// mm_dust_minier passes it) and the squeeze of the sequence's minimizers by them (mm_dust_minier, src/map.c:51-64). ONE WAVEFRONT per sequence; nothing
// crosses workgroups, every loop is bounded by the sequence length or by the capacity of a list.
//
// sdust_wave. The scan over the bases is the reference's automaton step by step (its state after base i depends on everything before); what is wide
// inside a step runs on the lanes:
//  - cw / cv (:136; 64 triplet values) are one register each, lane = triplet value; the window's triplets (kdq, at most 62, :73) a ring in a third,
//    lane = ring slot. A uniform index reads them with v_readlane, a one-lane select writes them;
//  - the list P of perfect intervals (by descending start) lives in LDS: start | finish | r << 8 | l, 12 B per entry. find_perfect's walk over the
//    entries with start >= the new one's (:117-121) takes 64 entries per step: they are a prefix of the list (a ballot finds its end) and the running
//    best ratio over them is folded record by record with ballots (a record = the first entry that beats the current best: exactly the entries at
//    which the reference's loop assigns). The shift that makes room (:125) moves 64 entries per step, from the top down; save_masked_regions' trim
//    (:104) is the same ballot from the tail.
// What the reference does and a tidy version would not (kept, see csrc/host/wm_sdust.h): the window's state survives an ambiguous base — only P, the
// run length and the current word are reset (:156-160) — and max_r / max_l are carried over all suffixes of one find_perfect call.
// P can grow to a few thousand entries (DESIGN.md "-T"): the list holds p_cap <= WM_SDUST_CAP entries; a sequence that needs more — or more result
// intervals than its slot holds — returns -1 and the caller finishes it on the host (host/wm_sdust.h), never from a truncated list.
//
// dust_filter_wave: 64 minimizers per step. The reference's interval cursor u only ever advances (map.c:54; with -H the spans vary and the starts are
// not monotone): per lane the first interval that ends behind the minimizer's start (binary search; the intervals are disjoint and ascending), then a
// wave max-scan with the carry of the steps before. The overlap is summed per lane from there (:57-61), the kept ones are compacted in place by a
// ballot: the write index never passes the read index.
#pragma once
#ifndef WM_DEV
#error "include simt.h before sdust_kernel.h"
#endif
#include "wm_internal.h"
#include "reads2bit.h"
#include "sketch_kernel.h"

#ifndef WM_SDUST_CAP
#define WM_SDUST_CAP 4096          // entries of the list of perfect intervals in LDS (48 KB)
#endif

namespace wmk {
using namespace simt;

constexpr int SDUST_W = 64, SDUST_KEEP = SDUST_W - 3 + 1;      // window length in bases; triplets in the window before the oldest leaves (:73)
constexpr int SDUST_LDS_INTS = 3 * WM_SDUST_CAP;

struct sdust_state {
	V<int> cw, cv, dq;                  // lane = triplet value (cw, cv) / ring slot (dq)
	int head, cnt, rw, rv, L, T;
	int *ps, *pf, *prl;                 // P in LDS: start, finish, r << 8 | l
	int n_p, p_cap, high;
	int *iv; int n_iv, iv_cap;          // results: (start, finish) pairs; the last one stays in res_st / res_en while it may still grow
	int res_st, res_en; bool have_res, overflow;
};

WM_DEV int sdust_ctz(uint64_t m) { return m == ~(uint64_t)0 ? 64 : __builtin_ctzll(~m); }     // length of the run of set bits from bit 0

// save_masked_regions (:92-106)
WM_DEV void sdust_retire(sdust_state &S, int win_start)
{
	if (S.n_p == 0) return;
	const int st = uniform(gld(S.ps, (long long)(S.n_p - 1)));
	if (st >= win_start) return;
	const int en = uniform(gld(S.pf, (long long)(S.n_p - 1)));
	const V<int> ln = lane();
	if (S.have_res && st <= S.res_en) { if (en > S.res_en) S.res_en = en; }
	else {
		if (S.have_res) {
			if (S.n_iv >= S.iv_cap) S.overflow = true;
			else {
				WM_IF(ln == 0) gst(S.iv, V<int>(2 * S.n_iv), V<int>(S.res_st)); gst(S.iv, V<int>(2 * S.n_iv + 1), V<int>(S.res_en)); WM_END
				++S.n_iv;
			}
		}
		S.res_st = st; S.res_en = en; S.have_res = true;
	}
	for (;;) {                          // drop the entries that start before the window: a run at the tail
		const V<int> idx = (S.n_p - 1) - ln;
		const vbool in = idx >= 0;
		V<int> s = 0x7fffffff;
		WM_IF(in) s = gld(S.ps, idx); WM_END
		const int run = sdust_ctz(ballot(in && s < win_start));
		S.n_p -= run;
		if (run < 64) break;
	}
}

// shift_window (:70-90)
WM_DEV void sdust_push(sdust_state &S, int t)
{
	const V<int> ln = lane();
	if (S.cnt >= SDUST_KEEP) {
		const int s = readlane(S.dq, S.head);
		S.head = (S.head + 1) & 63; --S.cnt;
		S.cw = S.cw - sel(ln == s, 1, 0);
		S.rw -= readlane(S.cw, s);
		if (S.L > S.cnt) {
			--S.L;
			S.cv = S.cv - sel(ln == s, 1, 0);
			S.rv -= readlane(S.cv, s);
		}
	}
	S.dq = sel(ln == ((S.head + S.cnt) & 63), t, S.dq);
	++S.cnt; ++S.L;
	S.rw += readlane(S.cw, t); S.cw = S.cw + sel(ln == t, 1, 0);
	S.rv += readlane(S.cv, t); S.cv = S.cv + sel(ln == t, 1, 0);
	if (readlane(S.cv, t) * 10 > S.T << 1) {
		int s;
		do {
			s = readlane(S.dq, (S.head + S.cnt - S.L) & 63);
			S.cv = S.cv - sel(ln == s, 1, 0);
			S.rv -= readlane(S.cv, s);
			--S.L;
		} while (s != t);
	}
}

// find_perfect (:108-132)
WM_DEV void sdust_perfect(sdust_state &S, int win_start)
{
	const V<int> ln = lane();
	V<int> c = S.cv;
	int r = S.rv, max_r = 0, max_l = 0;
	// j: entries scanned so far. The reference starts every suffix's walk at entry 0 (:117); the keys fall from suffix to suffix, so the entries a walk
	// passes are a growing prefix, an entry put in at its end belongs to every later one, and folding an entry twice changes nothing (the best ratio
	// already is at least its own, and only a strictly better one is taken): the walk resumes where the last one stopped
	int j = 0;
	for (int i = S.cnt - S.L - 1; i >= 0 && !S.overflow; --i) {
		const int t = readlane(S.dq, (S.head + i) & 63);
		r += readlane(c, t); c = c + sel(ln == t, 1, 0);
		const int new_l = S.cnt - i - 1;
		if (r * 10 <= S.T * new_l) continue;
		const int key = i + win_start;
		// the entries with start >= key, 64 per step; the best ratio among them and what was carried in (most suffixes pass no new entry: one word tells)
		while (j < S.n_p && uniform(gld(S.ps, (long long)j)) >= key) {
			const V<int> idx = ln + j;
			const vbool in = idx < S.n_p;
			V<int> st = -0x7fffffff - 1, rl = 0;
			WM_IF(in) st = gld(S.ps, idx); rl = gld(S.prl, idx); WM_END
			const int run = sdust_ctz(ballot(in && st >= key));
			const V<int> pr = rl >> 8, pl = rl & 255;
			const vbool inrun = ln < run;
			for (;;) {
				const uint64_t beats = ballot(inrun && ((pr * max_l > pl * max_r) || max_r == 0));
				if (!beats) break;
				const int p = __builtin_ctzll(beats);
				max_r = readlane(pr, p); max_l = readlane(pl, p);
			}
			j += run;
			if (run < 64) break;
		}
		if (max_r == 0 || r * max_l >= max_r * new_l) {
			max_r = r; max_l = new_l;
			if (S.n_p >= S.p_cap) { S.overflow = true; break; }
			for (int hi = S.n_p; hi > j; hi -= 64) {     // make room at j: 64 entries per step, the top ones first
				const V<int> idx = (hi - 1) - ln;
				const vbool mv = idx >= j;
				V<int> a = 0, b = 0, d = 0;
				WM_IF(mv) a = gld(S.ps, idx); b = gld(S.pf, idx); d = gld(S.prl, idx); WM_END
				lds_sync();
				WM_IF(mv) gst(S.ps, idx + 1, a); gst(S.pf, idx + 1, b); gst(S.prl, idx + 1, d); WM_END
				lds_sync();
			}
			WM_IF(ln == 0)
				gst(S.ps, V<int>(j), V<int>(key)); gst(S.pf, V<int>(j), V<int>(S.cnt + 2 + win_start)); gst(S.prl, V<int>(j), V<int>(r << 8 | new_l));
			WM_END
			lds_sync();
			++S.n_p;
			if (S.n_p > S.high) S.high = S.n_p;
		}
	}
}

// The masked intervals of one sequence of `len` codes — bytes at seqs + soff, or bases of the resident packed reads when soff carries
// WM_RD_PACKED_BIT (sk_code) — for threshold T > 0. lds: 3 * p_cap ints. (start, finish) pairs go to iv[0 .. 2 * iv_cap); returns how many, or -1
// when the list of perfect intervals or the result slot overflowed (iv is then incomplete). *high_out: the largest list held.
WM_DEV int sdust_wave(const uint8_t *seqs, const uint64_t *pk, const uint64_t *nm, long long soff, int len, int T, int *lds, int p_cap, int *iv, int iv_cap, int *high_out)
{
	const V<int> ln = lane();
	sdust_state S;
	S.cw = 0; S.cv = 0; S.dq = 0;
	S.head = S.cnt = S.rw = S.rv = S.L = 0; S.T = T;
	S.ps = lds; S.pf = lds + p_cap; S.prl = lds + 2 * p_cap;
	S.n_p = 0; S.p_cap = p_cap; S.high = 0;
	S.iv = iv; S.n_iv = 0; S.iv_cap = iv_cap;
	S.res_st = S.res_en = 0; S.have_res = false; S.overflow = false;
	int l = 0, t = 0;
	V<int> codes = 4;
	for (int i = 0; i <= len && !S.overflow; ++i) {      // :145-161
		if ((i & 63) == 0) {
			const V<int> p = ln + i;
			codes = 4;
			WM_IF(p < len) codes = sk_code(seqs, pk, nm, V<long long>(soff), cast<long long>(p)); WM_END
		}
		const int b = readlane(codes, i & 63);           // (the terminator at i == len reads as ambiguous)
		if (b < 4) {
			++l; t = (t << 2 | b) & 63;
			if (l >= 3) {
				const int start = (l - SDUST_W > 0 ? l - SDUST_W : 0) + (i + 1 - l);
				sdust_retire(S, start);
				sdust_push(S, t);
				if (S.rw * 10 > S.L * T) sdust_perfect(S, start);
			}
		} else {
			int start = (l - SDUST_W + 1 > 0 ? l - SDUST_W + 1 : 0) + (i + 1 - l);
			while (S.n_p > 0 && !S.overflow) {           // :158 — the calls that find the last entry inside the window do nothing: skip to the first that does not
				const int tail = uniform(gld(S.ps, (long long)(S.n_p - 1)));
				if (tail >= start) start = tail + 1;
				sdust_retire(S, start);
				++start;
			}
			l = 0; t = 0;
		}
	}
	if (S.have_res && !S.overflow) {
		if (S.n_iv >= S.iv_cap) S.overflow = true;
		else {
			WM_IF(ln == 0) gst(S.iv, V<int>(2 * S.n_iv), V<int>(S.res_st)); gst(S.iv, V<int>(2 * S.n_iv + 1), V<int>(S.res_en)); WM_END
			++S.n_iv;
		}
	}
	*high_out = S.high;
	return S.overflow ? -1 : S.n_iv;
}

// mm_dust_minier's squeeze (src/map.c:51-64) of a[0 .. n) in place by the n_iv intervals iv (pairs, ascending and disjoint); returns the new size
WM_DEV int dust_filter_wave(wm128_t *a, int n, const int *iv, int n_iv)
{
	const V<int> ln = lane();
	uint64_t *w = (uint64_t*)a;
	int k = 0, carry = 0;
	for (int j0 = 0; j0 < n; j0 += 64) {
		const V<int> j = ln + j0;
		const vbool in = j < n;
		V<uint64_t> x = (uint64_t)0, y = (uint64_t)0;
		WM_IF(in) x = gld(w, cast<long long>(j) * 2LL); y = gld(w, cast<long long>(j) * 2LL + 1LL); WM_END
		const V<int> qpos = cast<int>((y & (uint64_t)0xffffffffULL) >> 1), span = cast<int>(x & (uint64_t)0xff);
		const V<int> s = qpos - (span - 1), e = s + span;
		// the first interval that ends behind s (map.c:54 from interval 0) ...
		V<int> lo = 0, hi = n_iv;
		for (int it = 0; it < 32 && any(in && lo < hi); ++it) {
			WM_IF(in && lo < hi)
				const V<int> mid = (lo + hi) >> 1;
				const vbool before = gld(iv, mid * 2 + 1) <= s;
				lo = sel(before, mid + 1, lo);
				hi = sel(before, hi, mid);
			WM_END
		}
		// ... and from where the cursor stands: it never goes back
		const V<int> u = vmax(wave_scan_max(sel(in, lo, V<int>(0))), carry);
		carry = readlane(u, 63);
		V<int> v = u, covered = 0;
		vbool alive = in;
		for (int it = 0; it < n_iv; ++it) {              // map.c:57-61
			V<int> st = 0, en = 0;
			alive = alive && v < n_iv;
			WM_IF(alive) st = gld(iv, v * 2); en = gld(iv, v * 2 + 1); WM_END
			alive = alive && st < e;
			if (!any(alive)) break;
			WM_IF(alive)
				covered = covered + (vmin(e, en) - vmax(s, st));
				v = v + 1;
			WM_END
		}
		const vbool keep = in && covered <= (span >> 1);
		const uint64_t bm = ballot(keep);
		const V<int> at = mbcnt(bm) + k;
		WM_IF(keep) gst(w, cast<long long>(at) * 2LL, x); gst(w, cast<long long>(at) * 2LL + 1LL, y); WM_END
		k += popc64(bm);
	}
	return k;
}

} // namespace wmk

// wm_sdust.h — the reference's -T filter on the host: the symmetric-DUST intervals of a sequence (sdust_core, src/sdust.c:134-164, W = 64) and the
// squeeze of a minimizer list by them (mm_dust_minier, src/map.c:43-67). The device serves both (csrc/sdust_kernel.h); this restatement serves
// DeviceOps::window_batch's composed form (checker-backed ops in the test-suite) and the one job in a blue moon whose list of perfect intervals
// outgrows the device's (WM_SDUST_CAP entries): such a job is finished here, never by a truncated list.
//
// What a tidy restatement would get wrong, and this one keeps (sdust.c line numbers):
//  - an ambiguous base (or the end of the sequence) empties the list of perfect intervals and restarts the run length and the current word ONLY (:156-160):
//    the window's triplets, their counts cw / cv, rw, rv and L live on, while the window start of the next run is computed from the new run length
//    (:150). Intervals may therefore start or finish beyond the bases read so far, even beyond the sequence;
//  - find_perfect's best ratio (max_r / max_l) is carried over every suffix of ONE call, ties are inserted (>=), and a new interval goes behind every
//    entry with start >= its own (:117-128);
//  - save_masked_regions looks at the LAST entry only, merges it into the previous result when it touches or overlaps it, then drops every entry
//    that starts before the window (:96-105).
#pragma once
#include <stdint.h>
#include <vector>
#include "wm_core.h"

namespace wm {

struct DustIv { int32_t st, en; };             // a masked interval [st, en)

namespace sdust_detail {

struct Perfect { int st, en, r, l; };

struct Scan {
	enum { W = 64, WORDS = 64, KEEP = W - 3 + 1 };      // window length in bases, triplet values, triplets the window holds before the oldest leaves (:73)
	int T;
	int ring[64], head = 0, cnt = 0;                     // the window's triplets, oldest first (62 at most)
	int cw[WORDS] = {}, cv[WORDS] = {};                  // triplet counts of the window / of its suffix of L triplets
	int rw = 0, rv = 0, L = 0;
	std::vector<Perfect> P;                              // by descending start
	std::vector<DustIv> &res;
	size_t high = 0;
	Scan(int T_, std::vector<DustIv> &res_) : T(T_), res(res_) {}
	int at(int i) const { return ring[(head + i) & 63]; }

	void retire(int win_start)                           // :92-106
	{
		if (P.empty() || P.back().st >= win_start) return;
		const Perfect &p = P.back();
		if (!res.empty() && p.st <= res.back().en) { if (p.en > res.back().en) res.back().en = p.en; }
		else res.push_back({ p.st, p.en });
		size_t n = P.size();
		while (n > 0 && P[n - 1].st < win_start) --n;
		P.resize(n);
	}
	void push(int t)                                     // :70-90
	{
		if (cnt >= KEEP) {
			const int s = ring[head];
			head = (head + 1) & 63; --cnt;
			rw -= --cw[s];
			if (L > cnt) { --L; rv -= --cv[s]; }
		}
		ring[(head + cnt) & 63] = t; ++cnt;
		++L;
		rw += cw[t]++;
		rv += cv[t]++;
		if (cv[t] * 10 > T << 1) {
			int s;
			do {
				s = at(cnt - L);
				rv -= --cv[s];
				--L;
			} while (s != t);
		}
	}
	void perfect(int win_start)                          // :108-132
	{
		int c[WORDS], r = rv, max_r = 0, max_l = 0;
		for (int v = 0; v < WORDS; ++v) c[v] = cv[v];
		for (int i = cnt - L - 1; i >= 0; --i) {
			const int t = at(i);
			r += c[t]++;
			const int new_l = cnt - i - 1;
			if (r * 10 <= T * new_l) continue;
			size_t j = 0;
			for (; j < P.size() && P[j].st >= i + win_start; ++j)
				if (max_r == 0 || P[j].r * max_l > max_r * P[j].l) { max_r = P[j].r; max_l = P[j].l; }
			if (max_r == 0 || r * max_l >= max_r * new_l) {
				max_r = r; max_l = new_l;
				P.insert(P.begin() + (ptrdiff_t)j, Perfect{ i + win_start, cnt + 2 + win_start, r, new_l });
				if (P.size() > high) high = P.size();
			}
		}
	}
};

} // namespace sdust_detail

// the masked intervals of codes[0 .. len) (0..3 = A C G T, anything else ambiguous) for threshold T > 0; returns the largest number of perfect
// intervals held at once
inline int sdust_intervals(const uint8_t *codes, int len, int T, std::vector<DustIv> &out)
{
	out.clear();
	sdust_detail::Scan S(T, out);
	const int W = sdust_detail::Scan::W;
	int l = 0;
	unsigned t = 0;
	for (int i = 0; i <= len; ++i) {                     // :145-161
		const int b = i < len && codes[i] < 4 ? codes[i] : 4;
		if (b < 4) {
			++l; t = (t << 2 | (unsigned)b) & 63u;
			if (l >= 3) {
				const int start = (l - W > 0 ? l - W : 0) + (i + 1 - l);
				S.retire(start);
				S.push((int)t);
				if (S.rw * 10 > S.L * T) S.perfect(start);
			}
		} else {
			int start = (l - W + 1 > 0 ? l - W + 1 : 0) + (i + 1 - l);
			while (!S.P.empty()) S.retire(start++);
			l = 0; t = 0;
		}
	}
	return (int)S.high;
}

// mm_dust_minier's squeeze (src/map.c:51-64) of a[0 .. n) by the intervals of its sequence; returns the new size
inline int dust_filter(m128 *a, int n, const DustIv *iv, int n_iv)
{
	int k = 0, u = 0;                                    // u only ever advances: with varying spans (-H) the starts are not monotone
	for (int j = 0; j < n; ++j) {
		const int32_t qpos = (int32_t)((uint32_t)a[j].y >> 1), span = (int32_t)(a[j].x & 0xff);
		const int32_t s = qpos - (span - 1), e = s + span;
		while (u < n_iv && iv[u].en <= s) ++u;
		int covered = 0;
		for (int v = u; v < n_iv && iv[v].st < e; ++v)
			covered += (e < iv[v].en ? e : iv[v].en) - (s > iv[v].st ? s : iv[v].st);
		if (covered <= span >> 1) a[k++] = a[j];
	}
	return k;
}

// collect_minimizers' step for one sequence (src/map.c:80-81)
inline void dust_minimizers(std::vector<m128> &mini, const uint8_t *codes, int len, int T)
{
	if (T <= 0 || mini.empty()) return;
	std::vector<DustIv> iv;
	sdust_intervals(codes, len, T, iv);
	mini.resize((size_t)dust_filter(mini.data(), (int)mini.size(), iv.data(), (int)iv.size()));
}

} // namespace wm

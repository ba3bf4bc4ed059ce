// extra_kernel.h — the scan of mm_update_extra (src/align.c:240-286) over a region's FINAL CIGAR as an associative fold: dp_max, mlen, blen, n_ambi of
// wm_extra_walk (cigar_walk.h), cut into tiles that lanes, wavefronts and workgroups share. Written against the simt.h vocabulary only, so that the
// wavefront emulator runs the same text (tests/simt_emu/emu_extra.cpp).
//
// The fold. The CIGAR becomes a sequence of ELEMENTS: one per column of an M op (d = match, mismatch or ambi), one per I / D op (d = -(q + e * len)),
// none for an N op or an op code above 3. The reference's loop is  s <- max(0, s + d), max <- max(max, s)  per element (src/align.c:257-259, 268-269: the
// `else` of :259 and the missing update of :269 change nothing, max >= 0 and a gap only lowers s). A run of elements is therefore a function
//     s_in -> (s_out, peak) = (max(s_in + a, b), max(s_in + m, c))
// with a = sum of the d, b = s_out for s_in = 0 (>= 0), m = largest prefix sum (peak of the walk that never clamps), c = peak for s_in = 0 (>= 0):
//     one element   (a, b, m, c) = (d, 0, d, 0)
//     identity      (0, 0, -2^30, 0)
//     left, right   a = a1 + a2, b = max(b1 + a2, b2), m = max(m1, a1 + m2), c = max(c1, b1 + m2, c2)
// (substitute s_out of the left run into the right one: max(max(s + a1, b1) + a2, b2) = max(s + a1 + a2, b1 + a2, b2), and the peak is the larger of the left
// peak and max(max(s + a1, b1) + m2, c2)). The operator is associative and NOT commutative: every step of the wave reduction below composes "this lane, then the
// lane s to its right". dp_max of a region is c of the whole fold; mlen, blen, n_ambi are plain sums.
//
// int32 is exact: the entry points (wm_extra.hip) refuse a job whose max(|match|, |mismatch|, |ambi|) * (M columns) + sum (q + e * len) exceeds
// WM_EXTRA_MAX_ABS = 2^30. Every a, b, m, c of a run is a sum of d over a sub-run (or 0, or the identity's -2^30), so |a|, b, c, |m| <= 2^30, and a composition
// adds components of two DISJOINT runs (|sum| <= 2^30) or one component to the identity's m (>= -2^30 - 2^30 = INT32_MIN): nothing wraps.
//
// Column space. An M op has len columns, an I / D op max(1, ceil(len / 64)) — its element sits on the first, and every column counts the ambiguous bases of 64 bases
// of the gap, many bases per load (popcount of the ambiguity bitmap / word-wise byte and nibble tests) — an N op none. extra_prefix gives every op its first column,
// qoff and toff; a tile of tile_cols columns finds its first op by binary search, every lane folds tile_cols / 64 consecutive columns serially, one ordered wave
// reduction closes the tile. No lane walks a CIGAR, an M op or a gap longer than its share of a tile.
#pragma once
#include <stdint.h>
#include "../../include/wm_gpu.h"
#include "reads2bit.h"
#include "host/wm_final_plan.h"

#define WM_EXTRA_NEG (-0x40000000)          // m of the identity
// (WM_EXTRA_GAP — bases of an I / D op per column —, the job record wm_extra_djob_t and the host-side wm_extra_measure live with the batch planner: host/wm_final_plan.h)

namespace wmk {
using namespace simt;

// ---- operands -----------------------------------------------------------------------------------------------------------------------
// set bits of nm in the bit range [s, s + n), n <= 64 per lane
WM_DEV V<int> extra_nm_count(const uint64_t *nm, V<long long> s, V<int> n)
{
	const V<long long> e = s + cast<long long>(n), wi = s >> 6;
	V<int> cnt = 0;
	for (int k = 0; k < 2; ++k) {
		const V<long long> b0 = (wi + (long long)k) << 6;
		WM_IF(b0 < e)
			const V<uint64_t> x = gld(nm, wi + (long long)k);
			const V<int> lo = vmax(cast<int>(s - b0), 0), hi = vmin(cast<int>(e - b0), 64);
			const V<uint64_t> one = V<uint64_t>((uint64_t)1);
			const V<uint64_t> below_hi = sel(hi >= 64, V<uint64_t>(~(uint64_t)0), (one << (hi & 63)) - (uint64_t)1);
			const V<uint64_t> below_lo = (one << lo) - (uint64_t)1;
			cnt += vpopc64(x & below_hi & ~below_lo);
		WM_END
	}
	return cnt;
}

// the call's sequence slab: one byte per base, 8-byte aligned, readable to the end of the word that holds the last base
struct extra_src_bytes {
	const uint8_t *seqs; long long qb, tb;
	WM_DEV V<int> code(V<long long> p) const { return cast<int>(gld(seqs, p)); }
	WM_DEV V<int> q_code(V<int> i) const { return code(cast<long long>(i) + qb); }
	WM_DEV V<int> t_code(V<int> i) const { return code(cast<long long>(i) + tb); }
	// bytes above 3 in [s, s + n), n <= 64: eight bases per aligned load
	WM_DEV V<int> count(V<long long> s, V<int> n) const
	{
		const uint64_t *w = (const uint64_t*)seqs;
		const V<long long> e = s + cast<long long>(n), wi = s >> 3;
		V<int> cnt = 0;
		for (int k = 0; k < WM_EXTRA_GAP / 8 + 1; ++k) {
			const V<long long> b0 = (wi + (long long)k) << 3;
			if (!any(b0 < e)) break;
			WM_IF(b0 < e)
				const V<uint64_t> x = gld(w, wi + (long long)k);
				const V<uint64_t> h = x & (uint64_t)0xfcfcfcfcfcfcfcfcULL;          // bits 2..7 of a byte: the code is above 3
				const V<uint64_t> f = ((h | h >> 1 | h >> 2 | h >> 3 | h >> 4 | h >> 5) >> 2) & (uint64_t)0x0101010101010101ULL;
				const V<int> lo = vmax(cast<int>(s - b0), 0), hi = vmin(cast<int>(e - b0), 8);
				const V<uint64_t> one = V<uint64_t>((uint64_t)1);
				const V<uint64_t> below_hi = sel(hi >= 8, V<uint64_t>(~(uint64_t)0), (one << ((hi & 7) << 3)) - (uint64_t)1);
				const V<uint64_t> below_lo = (one << (lo << 3)) - (uint64_t)1;
				cnt += vpopc64(f & below_hi & ~below_lo);
			WM_END
		}
		return cnt;
	}
	WM_DEV V<int> q_ambi(V<int> i, V<int> n) const { return count(cast<long long>(i) + qb, n); }
	WM_DEV V<int> t_ambi(V<int> i, V<int> n) const { return count(cast<long long>(i) + tb, n); }
};

// what the device already holds: the resident read codes (reads2bit.h) in two-strand space — [0, L) forward, [L, 2L) reverse complement, outside N, the rule of
// wm_ksw_pos_t — and the 4-bit reference array S of the uploaded index (mm_idx_getseq, src/index.c:161-171). The packed words are read as they are.
struct extra_src_pos {
	const uint64_t *pk, *nm; const uint32_t *S; long long qb, tb; int q_pos, L;
	WM_DEV V<int> q_code(V<int> i) const
	{
		const V<int> p = i + q_pos;
		const vbool fw = p >= 0 && p < L, rv = p >= L && p < 2 * L;
		V<int> c = 4;
		WM_IF(fw || rv)
			const V<int> at = sel(fw, p, (2 * L - 1) - p);
			const V<int> r = rd2_code(pk, nm, cast<long long>(at) + qb);
			c = sel(rv && r < 4, 3 - r, r);
		WM_END
		return c;
	}
	WM_DEV V<int> t_code(V<int> i) const
	{
		const V<long long> p = cast<long long>(i) + tb;
		const V<uint32_t> w = gld(S, p >> 3);
		return cast<int>((w >> cast<int>((p & 7LL) << 2)) & (uint32_t)0xf);
	}
	// ambiguous bases of the two-strand range [i + q_pos, i + q_pos + n): N-ness survives the complement, so each strand's share is one bit range of the bitmap
	WM_DEV V<int> q_ambi(V<int> i, V<int> n) const
	{
		const V<int> p0 = i + q_pos, p1 = p0 + n;
		const V<int> f0 = vmin(vmax(p0, 0), L), f1 = vmin(vmax(p1, 0), L), r0 = vmin(vmax(p0, L), 2 * L), r1 = vmin(vmax(p1, L), 2 * L);
		V<int> cnt = n - (f1 - f0) - (r1 - r0);                                  // padding outside both strands
		cnt += extra_nm_count(nm, cast<long long>(f0) + qb, f1 - f0);
		cnt += extra_nm_count(nm, cast<long long>(2 * L - r1) + qb, r1 - r0);
		return cnt;
	}
	// nibbles above 3 in [i, i + n) of the target, n <= 64: eight bases per load
	WM_DEV V<int> t_ambi(V<int> i, V<int> n) const
	{
		const V<long long> s = cast<long long>(i) + tb, e = s + cast<long long>(n), wi = s >> 3;
		V<int> cnt = 0;
		for (int k = 0; k < WM_EXTRA_GAP / 8 + 1; ++k) {
			const V<long long> b0 = (wi + (long long)k) << 3;
			if (!any(b0 < e)) break;
			WM_IF(b0 < e)
				const V<uint32_t> x = gld(S, wi + (long long)k);
				const V<uint32_t> f = ((x >> 2) | (x >> 3)) & (uint32_t)0x11111111u;      // bit 2 or 3 of a nibble: the code is above 3
				const V<int> lo = vmax(cast<int>(s - b0), 0), hi = vmin(cast<int>(e - b0), 8);
				const V<uint32_t> one = V<uint32_t>((uint32_t)1);
				const V<uint32_t> below_hi = sel(hi >= 8, V<uint32_t>(~(uint32_t)0), (one << ((hi & 7) << 2)) - (uint32_t)1);
				const V<uint32_t> below_lo = (one << (lo << 2)) - (uint32_t)1;
				cnt += vpopc64(cast<uint64_t>(f & below_hi & ~below_lo));
			WM_END
		}
		return cnt;
	}
};

// ---- the operator ---------------------------------------------------------------------------------------------------------------------
// L <- L, then R (uniform values)
WM_DEV void extra_compose(int (&L)[4], const int (&R)[4])
{
	const int a = L[0] + R[0], b = vmax(L[1] + R[0], R[1]), m = vmax(L[2], L[0] + R[2]), c = vmax(vmax(L[3], L[1] + R[2]), R[3]);
	L[0] = a; L[1] = b; L[2] = m; L[3] = c;
}
// the ordered fold of the 64 lanes' tuples into lane 0: after the step with stride s lane j holds lanes [j, j + 2s) — LEFT is this lane, RIGHT the lane s above it
// (lanes beyond the wave contribute the identity)
WM_DEV void extra_wave_fold(V<int> &a, V<int> &b, V<int> &m, V<int> &c)
{
	for (int s = 1; s < 64; s <<= 1) {
		const V<int> a2 = shift_down(a, s, 0), b2 = shift_down(b, s, 0), m2 = shift_down(m, s, WM_EXTRA_NEG), c2 = shift_down(c, s, 0);
		const V<int> na = a + a2, nb = vmax(b + a2, b2), nm = vmax(m, a + m2), nc = vmax3(c, b + m2, c2);
		a = na; b = nb; m = nm; c = nc;
	}
}

// ---- pass 1: first column, qoff, toff of every op (entry n_cigar = the totals) ---------------------------------------------------------------
WM_DEV void extra_prefix(const uint32_t *cig, int n, int *colS, int *qS, int *tS)
{
	int cc = 0, cq = 0, ct = 0;
	for (int base = 0; base < n; base += 64) {
		const V<int> k = lane() + base;
		const vbool in = k < n;
		V<int> w = 0;
		WM_IF(in)
			w = cast<int>(gld(cig, k));
		WM_END
		const V<int> op = w & 0xf, len = lshr(w, 4);
		const vbool gap = op == 1 || op == 2;
		const V<int> cols = sel(op == 0, len, sel(in && gap, vmax(lshr(len + (WM_EXTRA_GAP - 1), 6), 1), V<int>(0)));
		const V<int> qa = sel(op == 0 || op == 1, len, 0), ta = sel(op == 0 || op == 2 || op == 3, len, 0);
		const V<int> ic = wave_scan_add(cols), iq = wave_scan_add(qa), it = wave_scan_add(ta);
		WM_IF(in)
			gst(colS, k, ic - cols + cc); gst(qS, k, iq - qa + cq); gst(tS, k, it - ta + ct);
		WM_END
		cc += readlane(ic, 63); cq += readlane(iq, 63); ct += readlane(it, 63);
	}
	WM_IF(lane() == 0)
		gst(colS, lane() + n, V<int>(cc)); gst(qS, lane() + n, V<int>(cq)); gst(tS, lane() + n, V<int>(ct));
	WM_END
}

// ---- one tile: columns [c_lo, c_lo + 64 * span) of a job -> o = { a, b, m, c, mlen, blen, n_ambi } (uniform) ----------------------------------------
template <class Src>
WM_DEV void extra_tile(const Src &S, const wm_extra_score_t &sc, const uint32_t *cig, const int *colS, const int *qS, const int *tS, int n_cigar, int ncols,
                       int c_lo, int span, int (&o)[7])
{
	const V<int> c0 = lane() * span + c_lo, cend = vmin(c0 + span, ncols);
	// the op that holds the lane's first column: colS[lo] <= c0 < colS[hi] throughout, so the op found has columns (zero-column ops are stepped over)
	const V<int> key = vmin(c0, ncols - 1);
	V<int> lo = 0, hi = n_cigar;
	for (int w = n_cigar; w > 1; w = (w + 1) >> 1) {
		const V<int> mid = (lo + hi) >> 1;
		const vbool act = (hi - lo) > 1, le = gld(colS, mid) <= key;
		lo = sel(act && le, mid, lo); hi = sel(act && !le, mid, hi);
	}
	V<int> k = lo;
	V<int> kst = gld(colS, k), kend = gld(colS, k + 1), w = cast<int>(gld(cig, k)), qb = gld(qS, k), tb = gld(tS, k);
	V<int> a = 0, b = 0, m = WM_EXTRA_NEG, c = 0, mlen = 0, blen = 0, namb = 0;
	for (int i = 0; i < span; ++i) {
		const V<int> col = c0 + i;
		const vbool act = col < cend;
		if (!any(act)) break;
		const V<int> k_was = k;
		while (any(act && col >= kend)) {
			WM_IF(act && col >= kend)
				k += 1;
				kend = gld(colS, k + 1);
			WM_END
		}
		WM_IF(k != k_was)
			kst = gld(colS, k); w = cast<int>(gld(cig, k)); qb = gld(qS, k); tb = gld(tS, k);
		WM_END
		const V<int> op = w & 0xf, len = lshr(w, 4), off = col - kst;
		const vbool gap = op == 1 || op == 2;
		V<int> d = 0;
		WM_IF(act && op == 0)
			const V<int> cq = S.q_code(qb + off), ct = S.t_code(tb + off);
			const vbool amb = cq > 3 || ct > 3, eq = cq == ct;
			d = sel(amb, sc.ambi, sel(eq, sc.match, sc.mismatch));
			namb += sel(amb, 1, 0); blen += sel(amb, 0, 1); mlen += sel(!amb && eq, 1, 0);
		WM_END
		WM_IF(act && gap)
			const V<int> g0 = off * WM_EXTRA_GAP, n = vmin(len - g0, WM_EXTRA_GAP);
			V<int> na = 0;
			WM_IF(op == 1)
				na = S.q_ambi(qb + g0, n);
			WM_ELSE
				na = S.t_ambi(tb + g0, n);
			WM_END
			namb += na; blen += n - na;
			d = sel(off == 0, 0 - (sc.e * len + sc.q), V<int>(0));
		WM_END
		// this lane's run, then the element (d, 0, d, 0)
		const vbool el = act && (op == 0 || (gap && off == 0));
		const V<int> ad = a + d, bd = b + d;
		m = sel(el, vmax(m, ad), m); c = sel(el, vmax(c, bd), c);
		a = sel(el, ad, a); b = sel(el, vmax(bd, 0), b);
	}
	extra_wave_fold(a, b, m, c);
	o[0] = readlane(a, 0); o[1] = readlane(b, 0); o[2] = readlane(m, 0); o[3] = readlane(c, 0);
	o[4] = readlane(wave_sum_i32(mlen), 0); o[5] = readlane(wave_sum_i32(blen), 0); o[6] = readlane(wave_sum_i32(namb), 0);
}

// lanes 0..5 store { dp_max, mlen, blen, n_ambi, qoff, toff } (wm_extra_res_t)
WM_DEV void extra_store_res(int *res, int dp_max, int mlen, int blen, int n_ambi, int qoff, int toff)
{
	const V<int> l = lane();
	const V<int> v = sel(l == 0, dp_max, sel(l == 1, mlen, sel(l == 2, blen, sel(l == 3, n_ambi, sel(l == 4, qoff, toff)))));
	WM_IF(l < 6)
		gst(res, l, v);
	WM_END
}

// ---- short class: one wavefront walks the job's tiles and carries the tuple in registers ------------------------------------------------------------
template <class Src>
WM_DEV void extra_short(const Src &S, const wm_extra_score_t &sc, const uint32_t *cig, const int *colS, const int *qS, const int *tS, int n_cigar, int tile_cols, int *res)
{
	const int ncols = uniform(gld(colS, (long long)n_cigar)), qoff = uniform(gld(qS, (long long)n_cigar)), toff = uniform(gld(tS, (long long)n_cigar));
	int T[4] = { 0, 0, WM_EXTRA_NEG, 0 }, mlen = 0, blen = 0, namb = 0;
	for (int c_lo = 0; c_lo < ncols; c_lo += tile_cols) {
		int o[7];
		extra_tile(S, sc, cig, colS, qS, tS, n_cigar, ncols, c_lo, tile_cols >> 6, o);
		const int R[4] = { o[0], o[1], o[2], o[3] };
		extra_compose(T, R);
		mlen += o[4]; blen += o[5]; namb += o[6];
	}
	extra_store_res(res, T[3], mlen, blen, namb, qoff, toff);
}

// ---- long class: one wavefront per tile writes its tuple and counts (8 ints), a combine pass folds them in order ---------------------------------------------
template <class Src>
WM_DEV void extra_long_tile(const Src &S, const wm_extra_score_t &sc, const uint32_t *cig, const int *colS, const int *qS, const int *tS, int n_cigar, int tile_cols, int tile, int *part)
{
	const int ncols = uniform(gld(colS, (long long)n_cigar));
	int o[7];
	extra_tile(S, sc, cig, colS, qS, tS, n_cigar, ncols, tile * tile_cols, tile_cols >> 6, o);
	const V<int> l = lane();
	const V<int> v = sel(l == 0, o[0], sel(l == 1, o[1], sel(l == 2, o[2], sel(l == 3, o[3], sel(l == 4, o[4], sel(l == 5, o[5], sel(l == 6, o[6], V<int>(0))))))));
	WM_IF(l < 8)
		gst(part, l, v);
	WM_END
}
WM_DEV void extra_combine(const int *part, int n_tiles, const int *qS, const int *tS, int n_cigar, int *res)
{
	const int qoff = uniform(gld(qS, (long long)n_cigar)), toff = uniform(gld(tS, (long long)n_cigar));
	int T[4] = { 0, 0, WM_EXTRA_NEG, 0 }, mlen = 0, blen = 0, namb = 0;
	for (int base = 0; base < n_tiles; base += 64) {
		const V<int> t = lane() + base;
		V<int> a = 0, b = 0, m = WM_EXTRA_NEG, c = 0, x4 = 0, x5 = 0, x6 = 0;
		WM_IF(t < n_tiles)
			const V<long long> at = cast<long long>(t) * 8LL;
			a = gld(part, at); b = gld(part, at + 1LL); m = gld(part, at + 2LL); c = gld(part, at + 3LL);
			x4 = gld(part, at + 4LL); x5 = gld(part, at + 5LL); x6 = gld(part, at + 6LL);
		WM_END
		extra_wave_fold(a, b, m, c);
		const int R[4] = { readlane(a, 0), readlane(b, 0), readlane(m, 0), readlane(c, 0) };
		extra_compose(T, R);
		mlen += readlane(wave_sum_i32(x4), 0); blen += readlane(wave_sum_i32(x5), 0); namb += readlane(wave_sum_i32(x6), 0);
	}
	extra_store_res(res, T[3], mlen, blen, namb, qoff, toff);
}

} // namespace wmk

// eqx_kernel.h — mm_update_cigar_eqx (src/align.c:169-238) over a region's FINAL CIGAR: every M op becomes its runs of '=' (7) and 'X' (8). The specification is
// wm_cigar_eqx (cigar_eqx.h); this is the same result as a per-column test, a segmented run-length fold and a variable-length write. Written against the simt.h
// vocabulary only, so that the wavefront emulator runs the same text (tests/simt_emu/emu_eqx.cpp). Operands come through extra_src_bytes / extra_src_pos (extra_kernel.h).
//
// Column space: the M columns only (an op of another code, or an M op of length 0, has none). eqx_prefix gives every op its first column (mS), qoff / toff (qS, tS; only
// codes 0..3 advance them, :186-192) and the number of ops of another code before it (cS). Per column c at offset j of its op:
//     e(c)    = the two codes are equal (N against N included, the reference's TODO at :179)
//     head(c) = j == 0 || e(c) != e(c - 1)          tail(c) = j == len - 1 || e(c) != e(c + 1)
// A run is [its head, its tail]; runs never cross an op boundary. The fold over columns is the tuple (number of heads, position of the last head): left then right is
// (h1 + h2, right has a head ? its last : the left's last) — associative and ordered; column positions only grow, so "the right's if it has one" is a maximum with -1 for
// "none", and both components are inclusive wave scans (wave_scan_add, wave_scan_max) with a carry from tile to tile. A run is EMITTED BY ITS TAIL: the carried last head
// is its start, whatever number of lanes or tiles (also tiles without any head) it spans.
//
// Two passes. COUNT: n_EQX = heads of the job; with n_M = n_cigar - cS[n_cigar] that decides the branch (src/align.c:195) and the output count, and eqx_job_scan gives
// every job its output offset. WRITE: in the rewrite branch the run whose tail is column c goes to slot (heads up to c) - 1 + cS[its op]; the last column of M op k
// leaves the heads up to there in gS[k], so that an op of another code lands at (largest gS before it) + cS[k] (eqx_ops_write: an exclusive max-scan over the ops, gS is 0
// where an op has no column). In the in-place branch eqx_ops_write alone relabels the M ops — THE QUIRK of :195-201, see cigar_eqx.h.
// Every lane folds tile_cols / 64 consecutive columns; no lane walks a CIGAR or an M op. Short jobs: one wavefront walks the tiles with the carry in registers; long jobs:
// one wavefront per tile, a combine pass turns the tiles' tuples into each tile's carry.
#pragma once
#include "extra_kernel.h"

namespace wmk {

// ---- pass 1: first M column, qoff, toff, ops of another code before it, for every op (entry n_cigar = the totals); gS = 0 ---------------------------------
WM_DEV void eqx_prefix(const uint32_t *cig, int n, int *mS, int *qS, int *tS, int *cS, int *gS)
{
	int cm = 0, cq = 0, ct = 0, cc = 0;
	for (int base = 0; base < n; base += 64) {
		const V<int> k = lane() + base;
		const vbool in = k < n;
		V<int> w = 0;
		WM_IF(in)
			w = cast<int>(gld(cig, k));
		WM_END
		const V<int> op = w & 0xf, len = lshr(w, 4);
		const V<int> cols = sel(op == 0, len, 0), other = sel(in && op != 0, 1, 0);
		const V<int> qa = sel(op == 0 || op == 1, len, 0), ta = sel(op == 0 || op == 2 || op == 3, len, 0);
		const V<int> im = wave_scan_add(cols), iq = wave_scan_add(qa), it = wave_scan_add(ta), ic = wave_scan_add(other);
		WM_IF(in)
			gst(mS, k, im - cols + cm); gst(qS, k, iq - qa + cq); gst(tS, k, it - ta + ct); gst(cS, k, ic - other + cc); gst(gS, k, V<int>(0));
		WM_END
		cm += readlane(im, 63); cq += readlane(iq, 63); ct += readlane(it, 63); cc += readlane(ic, 63);
	}
	WM_IF(lane() == 0)
		gst(mS, lane() + n, V<int>(cm)); gst(qS, lane() + n, V<int>(cq)); gst(tS, lane() + n, V<int>(ct)); gst(cS, lane() + n, V<int>(cc)); gst(gS, lane() + n, V<int>(0));
	WM_END
}

struct eqx_pre { const uint32_t *cig; const int *mS, *qS, *tS, *cS; int n_cigar, ncols; };
// the op that holds a lane's column: first / end column, the op word, qoff, toff, ops of another code before it
struct eqx_cur { V<int> k, kst, kend, w, qb, tb, cb; };
WM_DEV void eqx_load(const eqx_pre &P, eqx_cur &u)
{
	u.kst = gld(P.mS, u.k); u.w = cast<int>(gld(P.cig, u.k)); u.qb = gld(P.qS, u.k); u.tb = gld(P.tS, u.k); u.cb = gld(P.cS, u.k);
}
// mS[lo] <= c0 < mS[hi] throughout, so the op found has columns (ops without columns are stepped over); ncols > 0
WM_DEV eqx_cur eqx_seek(const eqx_pre &P, V<int> c0)
{
	const V<int> key = vmin(c0, P.ncols - 1);
	V<int> lo = 0, hi = P.n_cigar;
	for (int w = P.n_cigar; w > 1; w = (w + 1) >> 1) {
		const V<int> mid = (lo + hi) >> 1;
		const vbool act = (hi - lo) > 1, le = gld(P.mS, mid) <= key;
		lo = sel(act && le, mid, lo); hi = sel(act && !le, mid, hi);
	}
	eqx_cur u;
	u.k = lo; u.kend = gld(P.mS, lo + 1);
	eqx_load(P, u);
	return u;
}
// on to the op that holds col (col < ncols wherever act)
WM_DEV void eqx_step(const eqx_pre &P, eqx_cur &u, V<int> col, vbool act)
{
	const V<int> k_was = u.k;
	while (any(act && col >= u.kend)) {
		WM_IF(act && col >= u.kend)
			u.k += 1;
			u.kend = gld(P.mS, u.k + 1);
		WM_END
	}
	WM_IF(u.k != k_was)
		eqx_load(P, u);
	WM_END
}
template <class Src> WM_DEV V<int> eqx_equal(const Src &S, const eqx_cur &u, V<int> off) { return sel(S.q_code(u.qb + off) == S.t_code(u.tb + off), V<int>(1), V<int>(0)); }

// ---- one tile: columns [c_lo, c_lo + 64 * span) of a job -> o = { its heads, its last head or -1 } (uniform) -------------------------------------------
// EMIT: with the carry of everything before the tile (h_in heads, the last of them at lh_in) every tail writes its run to out, and every last column of an op its gS
template <class Src, bool EMIT>
WM_DEV void eqx_tile(const Src &S, const eqx_pre &P, int c_lo, int span, int h_in, int lh_in, uint32_t *out, int *gS, int (&o)[2])
{
	const V<int> c0 = lane() * span + c_lo, cend = vmin(c0 + span, P.ncols);
	const eqx_cur u0 = eqx_seek(P, c0);
	V<int> ep0 = 0;                                  // e of the column in front of the lane's first, where that is a column of the same op
	WM_IF(c0 < cend && c0 > u0.kst)
		ep0 = eqx_equal(S, u0, c0 - u0.kst - 1);
	WM_END
	eqx_cur u = u0;
	V<int> ep = ep0, hc = 0, lh = -1;
	for (int i = 0; i < span; ++i) {
		const V<int> col = c0 + i;
		const vbool act = col < cend;
		if (!any(act)) break;
		eqx_step(P, u, col, act);
		WM_IF(act)
			const V<int> off = col - u.kst, e = eqx_equal(S, u, off);
			const vbool head = off == 0 || e != ep;
			hc += sel(head, 1, 0); lh = sel(head, col, lh); ep = e;
		WM_END
	}
	const V<int> hi = wave_scan_add(hc), li = wave_scan_max(lh);
	o[0] = readlane(hi, 63); o[1] = readlane(li, 63);
	if (!EMIT) return;
	V<int> h = hi - hc + h_in, st = vmax(shr1(li, -1), lh_in);          // heads before the lane's first column; the last of them
	u = u0; ep = ep0;
	for (int i = 0; i < span; ++i) {
		const V<int> col = c0 + i;
		const vbool act = col < cend;
		if (!any(act)) break;
		eqx_step(P, u, col, act);
		WM_IF(act)
			const V<int> off = col - u.kst, last = lshr(u.w, 4) - 1, e = eqx_equal(S, u, off);
			const vbool head = off == 0 || e != ep;
			h += sel(head, 1, 0); st = sel(head, col, st); ep = e;
			V<int> tail = sel(off == last, 1, 0);
			WM_IF(off != last)
				tail = sel(eqx_equal(S, u, off + 1) != e, V<int>(1), V<int>(0));
			WM_END
			WM_IF(tail == 1)
				gst(out, h - 1 + u.cb, cast<uint32_t>(((col - st + 1) << 4) | sel(e == 1, V<int>(7), V<int>(8))));
			WM_END
			WM_IF(off == last)
				gst(gS, u.k, h);
			WM_END
		WM_END
	}
}

// ---- short class: one wavefront walks the job's tiles ---------------------------------------------------------------------------------------------------
// cnt = { n_EQX, n_cigar, ops of another code }
WM_DEV void eqx_store_cnt(int *cnt, int n_eqx, int n_cigar, int n_other)
{
	const V<int> l = lane();
	WM_IF(l < 3)
		gst(cnt, l, sel(l == 0, V<int>(n_eqx), sel(l == 1, V<int>(n_cigar), V<int>(n_other))));
	WM_END
}
template <class Src>
WM_DEV void eqx_short_count(const Src &S, const uint32_t *cig, const int *mS, const int *qS, const int *tS, const int *cS, int n_cigar, int tile_cols, int *cnt)
{
	const eqx_pre P = { cig, mS, qS, tS, cS, n_cigar, uniform(gld(mS, (long long)n_cigar)) };
	int H = 0;
	for (int c_lo = 0; c_lo < P.ncols; c_lo += tile_cols) {
		int o[2];
		eqx_tile<Src, false>(S, P, c_lo, tile_cols >> 6, 0, -1, 0, 0, o);
		H += o[0];
	}
	eqx_store_cnt(cnt, H, n_cigar, uniform(gld(cS, (long long)n_cigar)));
}
template <class Src>
WM_DEV void eqx_short_write(const Src &S, const uint32_t *cig, const int *mS, const int *qS, const int *tS, const int *cS, int n_cigar, int tile_cols, uint32_t *out, int *gS)
{
	const eqx_pre P = { cig, mS, qS, tS, cS, n_cigar, uniform(gld(mS, (long long)n_cigar)) };
	int H = 0, LH = -1;
	for (int c_lo = 0; c_lo < P.ncols; c_lo += tile_cols) {
		int o[2];
		eqx_tile<Src, true>(S, P, c_lo, tile_cols >> 6, H, LH, out, gS, o);
		H += o[0]; LH = vmax(LH, o[1]);
	}
}

// ---- long class: one wavefront per tile; part = 2 ints per tile -------------------------------------------------------------------------------------------
template <class Src>
WM_DEV void eqx_long_count(const Src &S, const uint32_t *cig, const int *mS, const int *qS, const int *tS, const int *cS, int n_cigar, int tile_cols, int tile, int *part)
{
	const eqx_pre P = { cig, mS, qS, tS, cS, n_cigar, uniform(gld(mS, (long long)n_cigar)) };
	int o[2];
	eqx_tile<Src, false>(S, P, tile * tile_cols, tile_cols >> 6, 0, -1, 0, 0, o);
	const V<int> l = lane();
	WM_IF(l < 2)
		gst(part, l, sel(l == 0, V<int>(o[0]), V<int>(o[1])));
	WM_END
}
// the tiles' { heads, last head } in order -> every tile's carry { heads before it, the last of them or -1 }, in place; and the job's cnt
WM_DEV void eqx_combine(int *part, int n_tiles, const int *cS, int n_cigar, int *cnt)
{
	int H = 0, LH = -1;
	for (int base = 0; base < n_tiles; base += 64) {
		const V<int> t = lane() + base;
		V<int> h = 0, lh = -1;
		WM_IF(t < n_tiles)
			h = gld(part, t * 2); lh = gld(part, t * 2 + 1);
		WM_END
		const V<int> hi = wave_scan_add(h), li = wave_scan_max(lh);
		WM_IF(t < n_tiles)
			gst(part, t * 2, hi - h + H); gst(part, t * 2 + 1, vmax(shr1(li, -1), LH));
		WM_END
		H += readlane(hi, 63); LH = vmax(LH, readlane(li, 63));
	}
	eqx_store_cnt(cnt, H, n_cigar, uniform(gld(cS, (long long)n_cigar)));
}
template <class Src>
WM_DEV void eqx_long_write(const Src &S, const uint32_t *cig, const int *mS, const int *qS, const int *tS, const int *cS, int n_cigar, int tile_cols, int tile, const int *part,
                           uint32_t *out, int *gS)
{
	const eqx_pre P = { cig, mS, qS, tS, cS, n_cigar, uniform(gld(mS, (long long)n_cigar)) };
	int o[2];
	eqx_tile<Src, true>(S, P, tile * tile_cols, tile_cols >> 6, uniform(gld(part, 0LL)), uniform(gld(part, 1LL)), out, gS, o);
}

// ---- the scan over jobs: cnt (3 ints per job) -> res (4 ints per job: wm_eqx_res_t = { off low, off high, n_cigar, in_place }), total[0] = ops of the whole call --------
// (one wavefront, 64 jobs per step; the entry points keep the sum below 2^31)
WM_DEV void eqx_job_scan(const int *cnt, int n_jobs, int *res, int *total)
{
	int off = 0;
	for (int base = 0; base < n_jobs; base += 64) {
		const V<int> j = lane() + base;
		V<int> n_eqx = 0, n = 0, other = 0;
		WM_IF(j < n_jobs)
			n_eqx = gld(cnt, j * 3); n = gld(cnt, j * 3 + 1); other = gld(cnt, j * 3 + 2);
		WM_END
		const vbool in_place = n_eqx == n - other;                    // n_EQX == n_M, src/align.c:195
		const V<int> n_out = sel(in_place, n, other + n_eqx), io = wave_scan_add(n_out);
		WM_IF(j < n_jobs)
			gst(res, j * 4, io - n_out + off); gst(res, j * 4 + 1, V<int>(0)); gst(res, j * 4 + 2, n_out); gst(res, j * 4 + 3, sel(in_place, V<int>(1), V<int>(0)));
		WM_END
		off += readlane(io, 63);
	}
	WM_IF(lane() == 0)
		gst(total, lane(), V<int>(off));
	WM_END
}

// ---- the ops of one job: the in-place branch (M -> =, :195-201), or the ops of another code of the rewrite branch (:233) --------------------------------------
WM_DEV void eqx_ops_write(const uint32_t *cig, int n, const int *cS, const int *gS, int in_place, uint32_t *out)
{
	int carry = 0;
	for (int base = 0; base < n; base += 64) {
		const V<int> k = lane() + base;
		const vbool in = k < n;
		V<int> w = 0, g = 0, cb = 0;
		WM_IF(in)
			w = cast<int>(gld(cig, k)); g = gld(gS, k); cb = gld(cS, k);
		WM_END
		const V<int> op = w & 0xf, gi = wave_scan_max(g), hb = vmax(shr1(gi, 0), carry);      // heads in front of op k
		if (in_place) {
			WM_IF(in)
				gst(out, k, cast<uint32_t>(sel(op == 0, (w & ~0xf) | 7, w)));
			WM_END
		} else {
			WM_IF(in && op != 0)
				gst(out, hb + cb, cast<uint32_t>(w));
			WM_END
		}
		carry = vmax(carry, readlane(gi, 63));
	}
}

} // namespace wmk

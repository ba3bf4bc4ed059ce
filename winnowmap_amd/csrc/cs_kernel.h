// cs_kernel.h — the bodies of the cs:Z / MD:Z tags (write_cs_core, write_MD_core, src/format.c:141-218) over a region's FINAL CIGAR. The specification is wm_cigar_cs
// (cigar_cs.h); this is the same text as a per-column classification, a fold over lanes and tiles, and a variable-length byte write. Written against the simt.h
// vocabulary only, so that the wavefront emulator runs the same text (tests/simt_emu/emu_cs.cpp). Operands come through extra_src_bytes / extra_src_pos (extra_kernel.h).
//
// Column space (HOW GAP BASES COUNT: every base of an I / D op that is printed is a column of its own, since it is a byte of its own — unlike the siblings' one
// column per 64 gap bases — and so it counts towards the columns that route a job, wm_extra_set_routing):
//     cs modes   an op of code 0 / 7 / 8: len base columns + 1 FLUSH column (the op's end, :162-167); I / D: 1 SIGN column + len base columns; N: 1 column
//     MD         an op of code 0 / 7 / 8: len base columns; D: 1 SIGN column ("<run>^") + len base columns; I and N: none (the run passes through them, :204, :212)
//     every mode one END column behind the last op (MD's final run, :216; it prints nothing in cs) — so a job has at least one column.
// cs_prefix gives every op (and the END pseudo-op n, word 15) its first column (cS), qoff / toff (qS, tS; codes 0, 7, 8 advance both, 1 the query, 2 and 3 the target)
// and a copy of its word (wS). A column is a MATCH (a base column of an M op whose two codes, clamped to 4, are equal) or not. With
//     last(c) = the last non-match column before c, or -1            run(c) = c - 1 - last(c)
// a non-match column prints the run in front of it, then its own bytes:
//     run text   cs short: ":<run>" if run > 0 (rk 1: every non-match column may be asked, the run is 0 behind anything but matches)
//                MD: "<run>", "0" included, in front of a mismatch and a SIGN (rk 2); "<run>" if run > 0 at END (rk 3); none at a D base (rk 0)    cs long: none (rk 0)
//     own bytes  mismatch "*tq" (cs) / "T" (MD); SIGN '+' / '-' / '^'; a gap base; N "~tt<len>tt"; FLUSH, END none
// and a match column prints nothing, except in cs long: its base, with '=' in front if it is the first column of its op or the column before it is a mismatch (the
// lane looks at that column itself). So THE TEXT OF A STRETCH OF COLUMNS IS A FUNCTION OF ITS OWN COLUMNS AND OF last() AT ITS FIRST COLUMN, and only the run text of
// the stretch's FIRST non-match column depends on that. The summary of a stretch is
//     (bytes without that one run text, first non-match column or -1, its rk, last non-match column or -1)
// and left-then-right is (b1 + b2 + [f2 >= 0 and l1 >= 0: rt(rk2, f2 - 1 - l1)], f1 >= 0 ? f1 : f2 (with its rk), max(l1, l2)) with the missing term kept open while
// l1 < 0 — associative and ordered. Column positions only grow, so last() is an inclusive wave_scan_max with a carry, and the bytes an inclusive wave_scan_add once
// every lane but the first with a non-match column has closed its term; digits(left.tail + right.head) of a run that crosses lanes or tiles (also tiles without any
// non-match column) is exactly that term. All of this is int32: the entry points refuse a job whose wm_cigar_cs_bound reaches 2^31.
//
// Passes. COUNT: every job's bytes; cs_job_scan gives every job its 64-bit offset. WRITE: the same walk again, every lane from its own byte offset, vector byte stores.
// Every lane folds tile_cols / 64 consecutive columns; no lane walks a CIGAR, an M op or a gap longer than its share of a tile. Short jobs: one wavefront walks the
// tiles with the carry in registers; long jobs: one wavefront per tile, a combine pass turns the tiles' summaries into each tile's carry.
#pragma once
#include "extra_kernel.h"
#include "cigar_cs.h"

namespace wmk {

WM_DEV V<int> cs_is_m(V<int> op) { return sel(op == 0 || op == 7 || op == 8, V<int>(1), V<int>(0)); }
// columns of an op (the rules above); op 15 = END
WM_DEV V<int> cs_op_cols(int mode, V<int> op, V<int> len)
{
	const vbool m = cs_is_m(op) == 1, gap = mode == WM_CS_MD ? op == 2 : (op == 1 || op == 2);
	V<int> c = sel(m, len + (mode == WM_CS_MD ? 0 : 1), 0);
	c = sel(gap, len + 1, c);
	c = sel(op == 3, V<int>(mode == WM_CS_MD ? 0 : 1), c);
	return sel(op == 15, V<int>(1), c);
}

// ---- pass 1: first column, qoff, toff and the word of every op k <= n (n = END); cS[n + 1] = the job's columns ------------------------------------------
WM_DEV void cs_prefix(int mode, const uint32_t *cig, int n, int *cS, int *qS, int *tS, int *wS)
{
	int cc = 0, cq = 0, ct = 0;
	for (int base = 0; base <= n; base += 64) {
		const V<int> k = lane() + base;
		const vbool in = k <= n;
		V<int> w = 15;
		WM_IF(k < n)
			w = cast<int>(gld(cig, k));
		WM_END
		const V<int> op = w & 0xf, len = lshr(w, 4), m = cs_is_m(op);
		const V<int> cols = sel(in, cs_op_cols(mode, op, len), 0);
		const V<int> qa = sel(in && (m == 1 || op == 1), len, 0), ta = sel(in && (m == 1 || op == 2 || op == 3), len, 0);
		const V<int> ic = wave_scan_add(cols), iq = wave_scan_add(qa), it = wave_scan_add(ta);
		WM_IF(in)
			gst(cS, k, ic - cols + cc); gst(qS, k, iq - qa + cq); gst(tS, k, it - ta + ct); gst(wS, k, w);
		WM_END
		cc += readlane(ic, 63); cq += readlane(iq, 63); ct += readlane(it, 63);
	}
	WM_IF(lane() == 0)
		gst(cS, lane() + (n + 1), V<int>(cc));
	WM_END
}

struct cs_pre { const int *cS, *qS, *tS, *wS; int n_ops, ncols, mode; };          // n_ops = n_cigar + 1 (END included), ncols >= 1
// the op that holds a lane's column: its index, first / end column, word, qoff, toff
struct cs_cur { V<int> k, kst, kend, w, qb, tb; };
WM_DEV void cs_load(const cs_pre &P, cs_cur &u)
{
	u.kst = gld(P.cS, u.k); u.w = gld(P.wS, u.k); u.qb = gld(P.qS, u.k); u.tb = gld(P.tS, u.k);
}
// cS[lo] <= c0 < cS[hi] throughout, so the op found has columns (ops without columns are stepped over)
WM_DEV cs_cur cs_seek(const cs_pre &P, V<int> c0)
{
	const V<int> key = vmin(c0, P.ncols - 1);
	V<int> lo = 0, hi = P.n_ops;
	for (int w = P.n_ops; w > 1; w = (w + 1) >> 1) {
		const V<int> mid = (lo + hi) >> 1;
		const vbool act = (hi - lo) > 1, le = gld(P.cS, mid) <= key;
		lo = sel(act && le, mid, lo); hi = sel(act && !le, mid, hi);
	}
	cs_cur u;
	u.k = lo; u.kend = gld(P.cS, lo + 1);
	cs_load(P, u);
	return u;
}
// on to the op that holds col (col < ncols wherever act)
WM_DEV void cs_step(const cs_pre &P, cs_cur &u, V<int> col, vbool act)
{
	const V<int> k_was = u.k;
	while (any(act && col >= u.kend)) {
		WM_IF(act && col >= u.kend)
			u.k += 1;
			u.kend = gld(P.cS, u.k + 1);
		WM_END
	}
	WM_IF(u.k != k_was)
		cs_load(P, u);
	WM_END
}

WM_DEV V<int> cs_digits(V<int> r)
{
	V<int> d = 1;
	int p = 10;
	for (int i = 0; i < 9; ++i) { d += sel(r >= p, 1, 0); if (i < 8) p *= 10; }
	return d;
}
// bytes of the run text of kind rk for a run of r
WM_DEV V<int> cs_rt_len(V<int> rk, V<int> r)
{
	const V<int> d = cs_digits(r);
	return sel(rk == 0, V<int>(0), sel(rk == 2, d, sel(r > 0, d + sel(rk == 1, V<int>(1), V<int>(0)), V<int>(0))));
}
WM_DEV V<int> cs_letter(V<int> code, bool up)          // "acgtn"[code] / "ACGTN"[code], code 0..4
{
	const V<uint64_t> tab = V<uint64_t>((uint64_t)0x6e74676361ULL);
	return cast<int>((tab >> (code << 3)) & (uint64_t)0xff) - (up ? 32 : 0);
}

// one column: match = 1 for a MATCH column; otherwise rk (the kind of run text in front of it) and own (bytes behind the run text); ch = up to three of its own bytes, low
// byte first (a match column's base in cs long; an intron's 5 + digits bytes are written by cs_tile itself)
struct cs_col { V<int> match, rk, own, ch; };
template <class Src>
WM_DEV cs_col cs_classify(const Src &S, const cs_pre &P, const cs_cur &u, V<int> col)
{
	const int mode = P.mode;
	const V<int> op = u.w & 0xf, len = lshr(u.w, 4), off = col - u.kst, m = cs_is_m(op);
	cs_col c;
	c.match = 0; c.rk = mode == WM_CS_SHORT ? 1 : 0; c.own = 0; c.ch = 0;
	WM_IF(m == 1 && off < len)
		const V<int> qc = vmin(S.q_code(u.qb + off), 4), tc = vmin(S.t_code(u.tb + off), 4);
		c.match = sel(qc == tc, V<int>(1), V<int>(0));
		if (mode == WM_CS_MD) { c.rk = 2; c.own = 1; c.ch = cs_letter(tc, true); }
		else { c.own = 3; c.ch = V<int>('*') | (cs_letter(tc, false) << 8) | (cs_letter(qc, false) << 16); }
		if (mode == WM_CS_LONG) c.ch = sel(c.match == 1, cs_letter(qc, true), c.ch);
	WM_END
	WM_IF(op == 1 || op == 2)
		c.own = 1;
		WM_IF(off == 0)
			c.ch = sel(op == 1, V<int>('+'), V<int>(mode == WM_CS_MD ? '^' : '-'));
			if (mode == WM_CS_MD) c.rk = 2;
		WM_ELSE
			V<int> b = 4;
			WM_IF(op == 1)
				b = S.q_code(u.qb + off - 1);
			WM_ELSE
				b = S.t_code(u.tb + off - 1);
			WM_END
			c.ch = cs_letter(vmin(b, 4), mode == WM_CS_MD);
		WM_END
	WM_END
	WM_IF(op == 3)
		c.own = cs_digits(len) + 5;
	WM_END
	if (mode == WM_CS_MD) c.rk = sel(op == 15, V<int>(3), c.rk);
	return c;
}
// is column off - 1 of the M op at u a MATCH (off >= 1)
template <class Src>
WM_DEV V<int> cs_match_at(const Src &S, const cs_cur &u, V<int> off)
{
	return sel(vmin(S.q_code(u.qb + off), 4) == vmin(S.t_code(u.tb + off), 4), V<int>(1), V<int>(0));
}
// decimal digits of v (n of them) at out[at ..]
WM_DEV void cs_put_digits(uint8_t *out, V<int> at, V<int> v, V<int> n, vbool act)
{
	for (int d = 0; d < 10; ++d) {
		const vbool go = act && n > d;
		if (!any(go)) break;
		WM_IF(go)
			gst(out, at + n - 1 - d, cast<uint8_t>(v % 10 + 48));
			v = v / 10;
		WM_END
	}
}

// ---- one tile: columns [c_lo, c_lo + 64 * span) of a job ------------------------------------------------------------------------------------------------
// CARRY: last() at the tile's first column is lh_in, o = { the tile's bytes, -, -, its last non-match column or -1 }; otherwise o = the tile's summary
// EMIT (with CARRY): b_in = the job's bytes in front of the tile; the tile's text goes to out
template <class Src, bool CARRY, bool EMIT>
WM_DEV void cs_tile(const Src &S, const cs_pre &P, int c_lo, int span, int b_in, int lh_in, uint8_t *out, int (&o)[4])
{
	const bool lng = P.mode == WM_CS_LONG;
	const V<int> c0 = lane() * span + c_lo, cend = vmin(c0 + span, P.ncols);
	const cs_cur u0 = cs_seek(P, c0);
	V<int> pm0 = 0;                                  // cs long: the column in front of the lane's first is a MATCH column of the same op
	if (lng) {
		WM_IF(c0 < cend && c0 > u0.kst && cs_is_m(u0.w & 0xf) == 1 && c0 - u0.kst <= lshr(u0.w, 4))
			pm0 = cs_match_at(S, u0, c0 - u0.kst - 1);
		WM_END
	}
	cs_cur u = u0;
	V<int> pm = pm0, bytes = 0, f = -1, frk = 0, lnm = -1;
	for (int i = 0; i < span; ++i) {
		const V<int> col = c0 + i;
		const vbool act = col < cend;
		if (!any(act)) break;
		cs_step(P, u, col, act);
		WM_IF(act)
			const cs_col c = cs_classify(S, P, u, col);
			WM_IF(c.match == 1)
				if (lng) bytes += sel(pm == 1 && col > u.kst, 1, 2);
			WM_ELSE
				bytes += c.own + sel(f >= 0, cs_rt_len(c.rk, col - 1 - lnm), V<int>(0));
				frk = sel(f >= 0, frk, c.rk); f = sel(f >= 0, f, col); lnm = col;
			WM_END
			pm = c.match;
		WM_END
	}
	const V<int> li = wave_scan_max(lnm), lprev = shr1(li, -1);
	const V<int> l_in = CARRY ? vmax(lprev, lh_in) : lprev;
	const vbool open = f >= 0 && !(CARRY || lprev >= 0);                   // the tile's first non-match column, its run text left open
	const V<int> tot = bytes + sel(f >= 0 && !open, cs_rt_len(frk, f - 1 - l_in), V<int>(0));
	const V<int> bi = wave_scan_add(tot);
	o[0] = readlane(bi, 63); o[3] = readlane(li, 63);
	o[1] = wave_max_i32(sel(open, f, V<int>(-1))); o[2] = wave_max_i32(sel(open, frk, V<int>(0)));
	if (!EMIT) return;
	V<int> at = bi - tot + b_in, last = l_in;
	u = u0; pm = pm0;
	for (int i = 0; i < span; ++i) {
		const V<int> col = c0 + i;
		const vbool act = col < cend;
		if (!any(act)) break;
		cs_step(P, u, col, act);
		WM_IF(act)
			const cs_col c = cs_classify(S, P, u, col);
			WM_IF(c.match == 1)
				if (lng) {
					WM_IF(!(pm == 1 && col > u.kst))
						gst(out, at, cast<uint8_t>(V<int>('=')));
						at += 1;
					WM_END
					gst(out, at, cast<uint8_t>(c.ch));
					at += 1;
				}
			WM_ELSE
				const V<int> r = col - 1 - last, n = cs_rt_len(c.rk, r);
				WM_IF(n > 0)
					V<int> nd = n;
					WM_IF(c.rk == 1)
						gst(out, at, cast<uint8_t>(V<int>(':')));
						nd = n - 1;
					WM_END
					cs_put_digits(out, at + (n - nd), r, nd, n > 0);
					at += n;
				WM_END
				const V<int> op = u.w & 0xf;
				WM_IF(op == 3)
					const V<int> len = lshr(u.w, 4), nd = cs_digits(len);
					gst(out, at, cast<uint8_t>(V<int>('~')));
					gst(out, at + 1, cast<uint8_t>(cs_letter(vmin(S.t_code(u.tb), 4), false)));
					gst(out, at + 2, cast<uint8_t>(cs_letter(vmin(S.t_code(u.tb + 1), 4), false)));
					cs_put_digits(out, at + 3, len, nd, op == 3);
					gst(out, at + nd + 3, cast<uint8_t>(cs_letter(vmin(S.t_code(u.tb + len - 2), 4), false)));
					gst(out, at + nd + 4, cast<uint8_t>(cs_letter(vmin(S.t_code(u.tb + len - 1), 4), false)));
				WM_ELSE
					WM_IF(c.own >= 1)
						gst(out, at, cast<uint8_t>(c.ch & 0xff));
					WM_END
					WM_IF(c.own == 3)
						gst(out, at + 1, cast<uint8_t>(lshr(c.ch, 8) & 0xff));
						gst(out, at + 2, cast<uint8_t>(lshr(c.ch, 16) & 0xff));
					WM_END
				WM_END
				at += c.own;
				last = col;
			WM_END
			pm = c.match;
		WM_END
	}
}

WM_DEV cs_pre cs_make_pre(int mode, const int *cS, const int *qS, const int *tS, const int *wS, int n_cigar)
{
	const cs_pre P = { cS, qS, tS, wS, n_cigar + 1, uniform(gld(cS, (long long)n_cigar + 1)), mode };
	return P;
}
WM_DEV void cs_store1(int *p, int v)
{
	WM_IF(lane() == 0)
		gst(p, lane(), V<int>(v));
	WM_END
}

// ---- short class: one wavefront walks the job's tiles -----------------------------------------------------------------------------------------------------
template <class Src>
WM_DEV void cs_short_count(const Src &S, int mode, const int *cS, const int *qS, const int *tS, const int *wS, int n_cigar, int tile_cols, int *cnt)
{
	const cs_pre P = cs_make_pre(mode, cS, qS, tS, wS, n_cigar);
	int B = 0, LH = -1;
	for (int c_lo = 0; c_lo < P.ncols; c_lo += tile_cols) {
		int o[4];
		cs_tile<Src, true, false>(S, P, c_lo, tile_cols >> 6, B, LH, 0, o);
		B += o[0]; LH = vmax(LH, o[3]);
	}
	cs_store1(cnt, B);
}
template <class Src>
WM_DEV void cs_short_write(const Src &S, int mode, const int *cS, const int *qS, const int *tS, const int *wS, int n_cigar, int tile_cols, uint8_t *out)
{
	const cs_pre P = cs_make_pre(mode, cS, qS, tS, wS, n_cigar);
	int B = 0, LH = -1;
	for (int c_lo = 0; c_lo < P.ncols; c_lo += tile_cols) {
		int o[4];
		cs_tile<Src, true, true>(S, P, c_lo, tile_cols >> 6, B, LH, out, o);
		B += o[0]; LH = vmax(LH, o[3]);
	}
}

// ---- long class: one wavefront per tile; part = 4 ints per tile ---------------------------------------------------------------------------------------------
template <class Src>
WM_DEV void cs_long_count(const Src &S, int mode, const int *cS, const int *qS, const int *tS, const int *wS, int n_cigar, int tile_cols, int tile, int *part)
{
	const cs_pre P = cs_make_pre(mode, cS, qS, tS, wS, n_cigar);
	int o[4];
	cs_tile<Src, false, false>(S, P, tile * tile_cols, tile_cols >> 6, 0, -1, 0, o);
	const V<int> l = lane();
	WM_IF(l < 4)
		gst(part, l, sel(l == 0, V<int>(o[0]), sel(l == 1, V<int>(o[1]), sel(l == 2, V<int>(o[2]), V<int>(o[3])))));
	WM_END
}
// the tiles' summaries in order -> every tile's carry { bytes in front of it, last() at its first column }, in place (ints 0 and 1 of its four); and the job's bytes
WM_DEV void cs_combine(int *part, int n_tiles, int *cnt)
{
	int B = 0, LH = -1;
	for (int base = 0; base < n_tiles; base += 64) {
		const V<int> t = lane() + base;
		V<int> b = 0, f = -1, frk = 0, l = -1;
		WM_IF(t < n_tiles)
			b = gld(part, t * 4); f = gld(part, t * 4 + 1); frk = gld(part, t * 4 + 2); l = gld(part, t * 4 + 3);
		WM_END
		const V<int> li = wave_scan_max(l), l_in = vmax(shr1(li, -1), LH);
		const V<int> tot = b + sel(f >= 0, cs_rt_len(frk, f - 1 - l_in), V<int>(0));
		const V<int> bi = wave_scan_add(tot);
		WM_IF(t < n_tiles)
			gst(part, t * 4, bi - tot + B); gst(part, t * 4 + 1, l_in);
		WM_END
		B += readlane(bi, 63); LH = vmax(LH, readlane(li, 63));
	}
	cs_store1(cnt, B);
}
template <class Src>
WM_DEV void cs_long_write(const Src &S, int mode, const int *cS, const int *qS, const int *tS, const int *wS, int n_cigar, int tile_cols, int tile, const int *part, uint8_t *out)
{
	const cs_pre P = cs_make_pre(mode, cS, qS, tS, wS, n_cigar);
	int o[4];
	cs_tile<Src, true, true>(S, P, tile * tile_cols, tile_cols >> 6, uniform(gld(part, 0LL)), uniform(gld(part, 1LL)), out, o);
}

// ---- the scan over jobs: cnt (bytes per job, < 2^31) -> res (4 ints per job: wm_cs_res_t = { off low, off high, len, 0 }), total = { low, high } of the call's bytes ----
// (one wavefront, 64 jobs per step; the offsets are 64-bit: the halves of every length are scanned apart, so no partial sum leaves int32)
WM_DEV void cs_job_scan(const int *cnt, int n_jobs, int *res, int *total)
{
	long long off = 0;
	for (int base = 0; base < n_jobs; base += 64) {
		const V<int> j = lane() + base;
		V<int> n = 0;
		WM_IF(j < n_jobs)
			n = gld(cnt, j);
		WM_END
		const V<int> lo = n & 0xffff, hi = lshr(n, 16), ilo = wave_scan_add(lo), ihi = wave_scan_add(hi);
		const V<long long> at = (cast<long long>(ihi - hi) << 16) + cast<long long>(ilo - lo) + off;
		WM_IF(j < n_jobs)
			gst(res, j * 4, cast<int>(at & 0xffffffffLL)); gst(res, j * 4 + 1, cast<int>(at >> 32)); gst(res, j * 4 + 2, n); gst(res, j * 4 + 3, V<int>(0));
		WM_END
		off += ((long long)readlane(ihi, 63) << 16) + (long long)readlane(ilo, 63);
	}
	WM_IF(lane() < 2)
		gst(total, lane(), sel(lane() == 0, V<int>((int)(off & 0xffffffffLL)), V<int>((int)(off >> 32))));
	WM_END
}

} // namespace wmk

// fix_kernel.h — mm_fix_cigar (src/align.c:91-167) over a region's stitched CIGAR by ONE wavefront, 64 ops per step; wm_fix_cigar (cigar_fix.h) is the specification.
// Written against the simt.h vocabulary only, so that the wavefront emulator runs the same text (tests/simt_emu/emu_fix.cpp). No LDS, no communication between
// workgroups, no polling; every loop is bounded by the job's op count or by a base count taken from the CIGAR.
//
// Pass 1 (left alignment, :98-124). At the start of every op the reference's qoff / toff equal the RAW CIGAR's prefix sums (a shift by l is undone when the grown M
// behind it is consumed), so extra_prefix's qS / tS are the offsets. An op k is ELIGIBLE when it is I or D, 0 < k < n - 1 and both neighbours are M: op codes only.
// Its shift is l_k = min(R_k, prev_len_k): R_k = the number of j >= 0 with seq[off - 1 - j] == seq[off + len - 1 - j] (query for an I, target for a D; 0..4 codes, N == N),
// prev_len_k = rawlen(k - 1) + l_(k-2), the last term only if op k - 2 is eligible. That is the only serial dependence, and it bites only when R_k reaches the whole raw
// M in front (a SATURATED op): every lane first compares up to rawlen(k - 1) bases of its own op; the saturated ops of the tile are then visited in order, each with its
// predecessor final, and the extra l_(k-2) bases are compared by the whole wavefront, 64 per step. l of the tile's last two ops is carried to the next tile.
// All reads stay inside the aligned stretch: l_k <= the M bases in front of k, so off - 1 - j >= 0, and off + len - 1 - j < off + len.
// After pass 1 every op is  raw + (l_(k-1) - l_(k+1)) << 4  (l = 0 where not eligible; an eligible neighbour implies this op is M). to_shrink: an op whose length is 0
// when the loop reaches it — raw + l_(k-1) == 0: a raw zero-length M right behind an eligible op that shifted has grown by then and does NOT count — or an eligible op
// with l_k == prev_len_k (prev_len_k == 0 included).
//
// Pass 2 (5I6D7I, :126-144) runs on pass 1's output with its zero-length ops in place. A MEMBER is an op that is I, D or of zero length; a start is a k <= n - 3 with
// op(k) in {1, 2} and op(k + 1) the other one. The reference's run goes from the first start of a stretch of members to the END of that stretch and the scan resumes behind
// it, so a stretch holds at most one run: the tiles are swept in order, the open run (start, both sums) is carried in uniform registers and closed — rewritten if it has
// more than two entries and both sums are positive — where the stretch ends. ((op 3, op 0) also passes the reference's trigger test; its run is empty: a no-op.)
//
// Squeeze, merge (:145-156, only if to_shrink) and the leading I / D (:157-166, ONE op) are one in-place sweep: a SEGMENT is a run of kept (non-zero) ops of one code, its
// head found with an ordered scan, its sum closed by the lane that holds the next head (or the carry at the end of the tile); the first segment's code decides whether
// everything lands one slot lower and its sum becomes qshift / tshift. A tile is loaded before it is stored and lands at or below its own indices. Sums wrap at 32 bits
// like the reference's; the entry points refuse a CIGAR whose lengths add up to 2^31 or more, so the ordered scans below see no wrap.
#pragma once
#include <stdint.h>
#include "extra_kernel.h"

namespace wmk {
using namespace simt;

template <class Src, class B>
WM_DEV V<int> fix_code(const Src &S, B is_q, V<int> i)
{
	V<int> c = 0;
	WM_IF(is_q)
		c = S.q_code(i);
	WM_ELSE
		c = S.t_code(i);
	WM_END
	return c;
}

// lanes 0..3 store { n_cigar, qshift, tshift, changed } (wm_fix_res_t)
WM_DEV void fix_store_res(int *res, int n, int qshift, int tshift, int changed)
{
	const V<int> l = lane();
	const V<int> v = sel(l == 0, n, sel(l == 1, qshift, sel(l == 2, tshift, changed)));
	WM_IF(l < 4)
		gst(res, l, v);
	WM_END
}

// pass 2: close the run [k0, b) with its sums
WM_DEV bool fix_close_run(uint32_t *out, int k0, int b, uint32_t s1, uint32_t s2)
{
	if (!(s1 > 0 && s2 > 0 && b - k0 > 2)) return false;
	for (int i0 = k0; i0 < b; i0 += 64) {
		const V<int> i = lane() + i0;
		WM_IF(i < b)
			const V<uint32_t> w = gld(out, i);
			gst(out, i, sel(i == k0, V<uint32_t>(s1 << 4 | 1u), sel(i == k0 + 1, V<uint32_t>(s2 << 4 | 2u), w & (uint32_t)0xf)));
		WM_END
	}
	return true;
}

// raw[0, n): the stitched CIGAR; qS / tS: extra_prefix of it; Ls: n ints of scratch; out: n ops of the output pool; res: wm_fix_res_t
template <class Src>
WM_DEV void fix_cigar_wave(const Src &S, const uint32_t *raw, int n, const int *qS, const int *tS, int *Ls, uint32_t *out, int *res)
{
	if (n <= 1) {
		WM_IF(lane() < n)
			gst(out, lane(), gld(raw, lane()));
		WM_END
		fix_store_res(res, n, 0, 0, 0);
		return;
	}
	bool shrink = false, moved = false;
	// ---- pass 1: l of every op -> Ls
	int carry0 = 0, carry1 = 0;                                          // l of the ops base - 2 and base - 1
	for (int base = 0; base < n; base += 64) {
		const V<int> k = lane() + base;
		const vbool in = k < n;
		V<int> w = 0, wp = 15, wn = 15, qo = 0, to = 0;
		WM_IF(in)
			w = cast<int>(gld(raw, k)); qo = gld(qS, k); to = gld(tS, k);
		WM_END
		WM_IF(in && k > 0)
			wp = cast<int>(gld(raw, k - 1));
		WM_END
		WM_IF(k + 1 < n)
			wn = cast<int>(gld(raw, k + 1));
		WM_END
		const V<int> op = w & 0xf, len = lshr(w, 4), prev = lshr(wp, 4);
		const vbool is_q = op == 1;
		const vbool elig = in && (op == 1 || op == 2) && k > 0 && k + 1 < n && (wp & 0xf) == 0 && (wn & 0xf) == 0;
		const V<int> off = sel(is_q, qo, to);
		V<int> l = 0;
		vbool go = elig && prev > 0;
		while (any(go)) {                                                // (at most rawlen(k - 1) rounds)
			WM_IF(go)
				const V<int> a = fix_code(S, is_q, off - 1 - l), b = fix_code(S, is_q, off + len - 1 - l);
				const vbool eq = a == b;
				l = sel(eq, l + 1, l);
				go = eq && l < prev;
			WM_END
		}
		// the saturated ops, in order: each with its predecessor final
		uint64_t sat = ballot(elig && l == prev);
		while (sat) {                                                    // (at most 64 rounds)
			const int s = __builtin_ctzll(sat);
			sat &= sat - 1;
			const int pl = s >= 2 ? readlane(l, s - 2) : s == 0 ? carry0 : carry1;
			if (pl == 0) { shrink = true; continue; }                    // l == prev_len
			const int s_off = readlane(off, s), s_len = readlane(len, s), s_prev = readlane(prev, s), cap = s_prev + pl;
			const bool s_q = readlane(op, s) == 1;
			int ls = s_prev;
			while (ls < cap) {                                           // (l_(k-2) more bases, 64 per step)
				const V<int> j = lane() + ls;
				V<int> a = 0, b = 0;
				WM_IF(j < cap)
					a = fix_code(S, s_q, s_off - 1 - j); b = fix_code(S, s_q, s_off + s_len - 1 - j);
				WM_END
				const uint64_t ne = ballot(j < cap && a != b);
				if (ne) { ls += __builtin_ctzll(ne); break; }
				ls = vmin(ls + 64, cap);
			}
			if (ls == cap) shrink = true;
			l = sel(lane() == s, V<int>(ls), l);
		}
		if (any(l > 0)) moved = true;
		// (the reference tests an op's length when it reaches it: an M behind an eligible op has grown by that op's shift by then)
		if (any(in && len + shr1(l, carry1) == 0)) shrink = true;
		WM_IF(in)
			gst(Ls, k, l);
		WM_END
		carry0 = readlane(l, 62); carry1 = readlane(l, 63);
	}
	mem_sync();
	// ---- pass 1's output -> out
	for (int base = 0; base < n; base += 64) {
		const V<int> k = lane() + base;
		V<int> la = 0, lb = 0;
		WM_IF(k < n && k > 0)
			la = gld(Ls, k - 1);
		WM_END
		WM_IF(k + 1 < n)
			lb = gld(Ls, k + 1);
		WM_END
		WM_IF(k < n)
			gst(out, k, gld(raw, k) + (cast<uint32_t>(la) << 4) - (cast<uint32_t>(lb) << 4));
		WM_END
	}
	mem_sync();
	// ---- pass 2
	if (n > 2) {
		bool open = false;
		int k0 = 0;
		uint32_t s1 = 0, s2 = 0;
		for (int base = 0; base < n; base += 64) {
			const V<int> k = lane() + base;
			const vbool in = k < n;
			V<int> w = 0x1f, wn = 15;                                    // (beyond the CIGAR: no member)
			WM_IF(in)
				w = cast<int>(gld((const uint32_t*)out, k));
			WM_END
			WM_IF(k + 1 < n)
				wn = cast<int>(gld((const uint32_t*)out, k + 1));
			WM_END
			const V<int> op = w & 0xf, len = lshr(w, 4);
			const vbool indel = op == 1 || op == 2;
			const uint64_t memB = ballot(in && (indel || len == 0)), trigB = ballot(in && indel && k + 2 < n && (wn & 0xf) == 3 - op);
			int pos = 0;
			while (pos < 64) {                                           // (at most one round per run of the tile, plus one)
				if (!open) {
					const uint64_t t = trigB >> pos;
					if (!t) break;
					pos += __builtin_ctzll(t);
					open = true; k0 = base + pos; s1 = s2 = 0;
				}
				const uint64_t nm = ~memB >> pos;
				const int e = nm ? pos + __builtin_ctzll(nm) : 64;
				const vbool inr = lane() >= pos && lane() < e;
				s1 += (uint32_t)readlane(wave_sum_i32(sel(inr && op == 1, len, V<int>(0))), 0);
				s2 += (uint32_t)readlane(wave_sum_i32(sel(inr && op == 2, len, V<int>(0))), 0);
				if (e < 64) {
					if (fix_close_run(out, k0, base + e, s1, s2)) shrink = true;
					open = false; pos = e + 1;
				} else pos = 64;
			}
		}
		if (open && fix_close_run(out, k0, n, s1, s2)) shrink = true;
		mem_sync();
	}
	// ---- squeeze + merge (if shrink), the leading I / D
	int n_seg = 0, cur_op = 0, lead = -1, op0 = 0, shift = 0;
	bool have = false;
	uint32_t cur_sum = 0;
	for (int base = 0; base < n; base += 64) {
		const V<int> k = lane() + base;
		const vbool in = k < n;
		V<int> w = 0;
		WM_IF(in)
			w = cast<int>(gld((const uint32_t*)out, k));
		WM_END
		const V<int> op = w & 0xf, len = lshr(w, 4);
		const vbool kept = in && (!shrink || len != 0);
		const V<int> sc = wave_scan_max(sel(kept, ((lane() + 1) << 4) | op, V<int>(-1)));      // the last kept op at or below this lane
		const V<int> prev = vmax(shr1(sc, -1), have ? cur_op : -1);
		const vbool head = kept && (!shrink || prev < 0 || (prev & 0xf) != op);
		const uint64_t headB = ballot(head);
		if (!headB) {                                                    // the tile continues the open segment, or holds nothing
			if (have) cur_sum += (uint32_t)readlane(wave_sum_i32(sel(kept, len, V<int>(0))), 0);
			continue;
		}
		if (lead < 0) { op0 = readlane(op, __builtin_ctzll(headB)); lead = op0 == 1 || op0 == 2 ? 1 : 0; }
		const V<int> seg = mbcnt(headB) + sel(head, 1, 0) + (n_seg - 1);                          // the segment of a kept lane
		const V<int> klen = sel(kept, len, V<int>(0)), P = wave_scan_add(klen), Pex = P - klen;
		const V<int> hp = wave_scan_max(sel(head, Pex, V<int>(-1)));                              // Pex of the last head at or below this lane
		const V<int> start = shr1(hp, -1);
		// a head closes the segment in front of it
		const vbool closes = head && seg > 0;
		const V<uint32_t> psum = sel(start >= 0, cast<uint32_t>(Pex - start), cast<uint32_t>(Pex) + cur_sum);
		const uint64_t firstB = ballot(closes && seg == 1);
		if (firstB && lead == 1) shift = (int)readlane(cast<int>(psum), __builtin_ctzll(firstB));
		WM_IF(closes && seg - 1 - lead >= 0)
			gst(out, seg - 1 - lead, (psum << 4) | cast<uint32_t>(prev & 0xf));
		WM_END
		// the tile's last segment stays open
		const int last_start = readlane(hp, 63), p_all = readlane(P, 63);
		cur_sum = (uint32_t)(p_all - last_start);
		cur_op = readlane(sc, 63) & 0xf; have = true;
		n_seg += popc64(headB);
	}
	if (lead < 0) lead = 0;
	if (have) {
		if (n_seg == 1 && lead == 1) shift = (int)cur_sum;
		else {
			WM_IF(lane() == 0)
				gst(out, lane() + (n_seg - 1 - lead), V<uint32_t>(cur_sum << 4 | (uint32_t)cur_op));
			WM_END
		}
	}
	fix_store_res(res, n_seg - lead, lead == 1 && op0 == 1 ? shift : 0, lead == 1 && op0 == 2 ? shift : 0, moved || shrink || lead == 1 ? 1 : 0);
}

} // namespace wmk

// ll_kernel.h — ksw_ll_qinit + ksw_ll_i16 (src/ksw2.h:82-83, src/ksw2_ll_sse.c:32-147) for gfx950, one wavefront per job: the local-alignment score with the end
// coordinates of the striped machine, bit for bit what wm_ksw_ll_spec (ksw_ll.h, the specification) returns for gapo > 0. Written against simt.h; the wavefront
// emulator runs the same text (tests/simt_emu/emu_ll.cpp).
//
// The striped machine in position terms (p = query position, 0 <= p < n = 8 * slen; segment l = [l * slen, (l + 1) * slen); oe = gapo + gape, ext = gape; all values
// clamped at 0 from below, the add at 32767 from above). Per target row i:
//     D[p]      = max(min(H[i-1][p-1] + S[t_i][p], 32767), E[p])                  S = 0 on the pad positions p >= qlen, H[.][-1] = H[-1][.] = 0
//     Fseg[p]   = 0 at a segment start, else max(Fseg[p-1] - ext, Hmain[p-1] - oe)   the F of the main loop: it never crosses a segment boundary
//     Ffull[p]  = 0 at p = 0,           else max(Ffull[p-1] - ext, H[p-1] - oe)      ... and what the lazy-F rounds add to it
//     Hmain[p]  = max(D[p], Fseg[p])       the main loop's H: the next row's E is opened from it, and the row maximum is taken over it
//     H[p]      = max(D[p], Ffull[p])      the corrected H: the next row's diagonal
//     E'[p]     = max(E[p] - ext, Hmain[p] - oe)
// score = the largest Hmain; te = the last row that holds it; qe = the position of row te with Hmain == score whose striped slot (p % slen) * 8 + p / slen is largest
// (in row te, H[p] == score iff Hmain[p] == score). With gapo = 0 the specification's lazy-F loop leaves early and drops F values that tie; the entry points refuse it.
//
// Every term of cell (i, p) that comes from the left comes from cell (i, p - 1): an anti-diagonal wavefront. Lane L owns position base + L of a PASS of 64 positions
// and works on row s - L at step s; H, Fseg, Ffull and the row's target code move one lane to the right per step (four DPP wave_shr:1 moves), E stays in its lane.
// No row is stored: every lane keeps the best Hmain of its column and the last row that reached it, packed with the slot into one 64-bit key; one wave maximum at
// the end gives {score, te, qe}. Target codes are fetched 64 rows at a time (one per lane) and handed to lane 0 by v_readlane.
//   * register class (HAND = false): n <= 64, one pass, no memory but the operands;
//   * LDS class (HAND = true): ceil(n / 64) passes; lane 63 leaves {H, Fseg out, Ffull out} of every row of its column in LDS (two ints per row, in place: row i is
//     read at step i - i % 64 and rewritten at step i + 63), the next pass's lane 0 takes them 64 rows at a time. One wavefront per workgroup, so DS order is enough.
// Stores: the three result words, plain vector stores.
#pragma once
#include <stdint.h>
#include "../../include/wm_gpu.h"
#include "reads2bit.h"

namespace wmk {
using namespace simt;

constexpr int LL_V = 8;   // int16 lanes of the reference's vector: the query is padded to a multiple of it, and its positions are cut into that many segments

// a per-lane LDS load (the emulator's lds_ld takes a uniform index only)
#ifdef WM_SIMT_EMU
WM_DEV V<int> ll_lds_ld(const int *p, V<int> i) { return gld(p, i); }
#else
WM_DEV V<int> ll_lds_ld(const int *p, V<int> i) { return lds_ld(p, (long long)i); }
#endif

// operands as 0..4 codes in the call's byte slab: element i of the query is seqs[qb + i * step], of the target seqs[tb + i * step]; codes above 4 count as 4
struct ll_src_bytes {
	const uint8_t *seqs; long long qb, tb; int step;
	WM_DEV V<int> q_code(V<int> i) const { return vmin(cast<int>(gld(seqs, cast<long long>(i) * (long long)step + qb)), 4); }
	WM_DEV V<int> t_code(V<int> i) const { return vmin(cast<int>(gld(seqs, cast<long long>(i) * (long long)step + tb)), 4); }
};
// operands as positions (wm_ksw_pos_t): query element i = index q_pos + i * step of the two-strand space of the (sub)read at qb, L long ([0, L) forward, [L, 2L)
// reverse complement, outside N); target element i = base tb + i * step of the packed reference (4 bits per base)
struct ll_src_pos {
	const uint64_t *pk, *nm; const uint32_t *S; long long qb, tb; int q_pos, L, step;
	WM_DEV V<int> q_code(V<int> i) const
	{
		const V<int> p = i * step + q_pos;
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
		const V<long long> p = cast<long long>(i) * (long long)step + tb;
		const V<uint32_t> w = gld(S, p >> 3);
		return vmin(cast<int>((w >> cast<int>((p & 7LL) << 2)) & (uint32_t)0xf), 4);
	}
};

// One job by one wavefront. mat: the 5 x 5 matrix widened to 25 ints (row = target code); rows: HAND only, 2 * tlen ints of LDS; out3 = {score, qe, te}.
template <bool HAND, class Src>
WM_DEV void ll_job(const Src &src, int qlen, int tlen, const int *mat, int oe, int ext, int *rows, int *out3)
{
	const int slen = (qlen + LL_V - 1) / LL_V, n = slen * LL_V;
	const int n_pass = (n + 63) / 64;
	WM_EMU_ASSERT(HAND || n_pass == 1);
	const V<int> ln = lane();
	V<long long> key = -1LL;                                               // (best Hmain << 48 | last row that reached it << 24 | striped slot) over this lane's columns
	for (int pass = 0; pass < n_pass; ++pass) {
		const int base = pass * 64;
		const int lanes = n - base < 64 ? n - base : 64;                    // columns of this pass
		const bool first = pass == 0, last = pass == n_pass - 1;
		const V<int> p = ln + base;
		const vbool col = p < n;
		const V<int> seg = p / slen, j = p - seg * slen;
		const vbool seg_start = j == 0;
		// this column's five scores, biased by 128: four in one register, S[4] in another; a pad column scores 0
		V<int> sc03 = (int)0x80808080u, sc4 = 128;
		WM_IF(p < qlen)
			const V<int> qc = src.q_code(p);
			sc03 = (gld(mat, qc) + 128) | (gld(mat, qc + 5) + 128) << 8 | (gld(mat, qc + 10) + 128) << 16 | (gld(mat, qc + 15) + 128) << 24;
			sc4 = gld(mat, qc + 20) + 128;
		WM_END
		V<int> E = 0, H = 0, fs_out = 0, ff_out = 0, hl = 0, tc = 0, best = -1, brow = 0;
		V<int> t64 = 0, hf64 = 0, ff64 = 0;                                  // the next 64 rows: target codes, and the left neighbour pass's {H | Fseg << 16}, Ffull
		const int n_step = tlen + lanes - 1;
		for (int s = 0; s < n_step; ++s) {
			const int k = s & 63;
			if (k == 0) {
				WM_KEEP_BRANCH();
				const V<int> r = ln + s;
				WM_IF(r < tlen)
					t64 = src.t_code(r);
					if (HAND && !first) { hf64 = ll_lds_ld(rows, r * 2); ff64 = ll_lds_ld(rows, r * 2 + 1); }
				WM_END
			}
			// what row s of the column left of this pass hands to lane 0 (nothing in front of the first pass; rows >= tlen are never used)
			const int hf_in = HAND && !first ? readlane(hf64, k) : 0, ff_in0 = HAND && !first ? readlane(ff64, k) : 0;
			const V<int> diag = hl;                                          // H[i-1][p-1]: what arrived one step ago
			hl = shr1(H, V<int>(hf_in & 0xffff));                            // H[i][p-1]
			const V<int> fs_in = sel(seg_start, V<int>(0), shr1(fs_out, V<int>(lshr(hf_in, 16))));
			const V<int> ff_in = shr1(ff_out, V<int>(ff_in0));
			tc = shr1(tc, V<int>(readlane(t64, k)));
			const V<int> i = s - ln;
			const vbool valid = col && i >= 0 && i < tlen;
			const V<int> sc = sel(tc < 4, (sc03 >> (vmin(tc, 3) << 3)) & 0xff, sc4) - 128;
			const V<int> d = vmax(vmin(diag + sc, 32767), E);
			const V<int> hmain = vmax(d, fs_in), h = vmax(d, ff_in);
			const V<int> open = hmain - oe;
			E = sel(valid, vmax3(E - ext, open, V<int>(0)), E);
			fs_out = sel(valid, vmax3(fs_in - ext, open, V<int>(0)), fs_out);
			ff_out = sel(valid, vmax3(ff_in - ext, h - oe, V<int>(0)), ff_out);
			H = sel(valid, h, H);
			const vbool up = valid && hmain >= best;                          // >=: the last row that reaches the column's best
			best = sel(up, hmain, best);
			brow = sel(up, i, brow);
			if (HAND && !last) {
				WM_IF(ln == 63 && valid)
					lds_st(rows, i * 2, H | fs_out << 16);
					lds_st(rows, i * 2 + 1, ff_out);
				WM_END
			}
		}
		const V<long long> kp = cast<long long>(vmax(best, 0)) << 48 | cast<long long>(brow) << 24 | cast<long long>(j * LL_V + seg);
		key = sel(col && best >= 0 && kp > key, kp, key);
	}
	const long long top = uniform(wave_max_i64(key));
	const int slot = (int)(top & 0xffffff);
	gst(out3, 0LL, (int)(top >> 48));
	gst(out3, 1LL, slot / LL_V + slot % LL_V * slen);
	gst(out3, 2LL, (int)(top >> 24 & 0xffffff));
}

} // namespace wmk

// ksw_ll.h — ksw_ll_qinit + ksw_ll_i16 (src/ksw2.h:82-83, src/ksw2_ll_sse.c:32-147), the striped local-alignment SCORE with end coordinates, written ONCE as a literal
// lane-by-lane loop over plain arrays (8 x int16 per vector, m = 5). The host mapper compiles it (host/wm_align.cpp: wm::ll_i16_portable, the specification of its SSE
// twin), and it is the SPECIFICATION of the device form (ll_kernel.h behind wm_ksw_ll_batch / wm_ksw_ll_batch_pos). It is not textbook Smith-Waterman; what the striped
// machine lets a caller observe, and what every other form has to reproduce:
//   * the query is padded to n = 8 * slen positions, slen = ceil(qlen / 8); pad positions score 0 against everything and H travels into them along the diagonal, so the
//     best cell may sit on a pad slot and *qe >= qlen (mm_align1_inv turns that into a start up to 7 bases in front of the gap, src/align.c:826-828);
//   * H is a saturating int16 add (scores reach 32767); the gap subtractions are unsigned-saturating (they clamp at 0); E, F and H are never negative;
//   * E of the next row is opened from the MAIN-LOOP H, which holds only the F that stayed inside one of the 8 striped segments [l * slen, (l + 1) * slen); the lazy-F
//     rounds correct H, never E;
//   * the row maximum is taken over the main-loop H, pads included; *te is the LAST row whose maximum is >= the running best (so the last row when the score is 0);
//   * *qe is the LAST slot in striped storage order (slot = (p % slen) * 8 + p / slen) of row *te whose corrected H equals the score — not the largest position.
// Query position p lives in vector j = p % slen, lane l = p / slen. gapo + gape must fit an int16; gapo = 0 is accepted (the early exit of the lazy-F loop then drops
// F values that tie, which no closed form reproduces — the mapper never has it, src/options.c:166-176).
#pragma once
#include <stdint.h>
#include <vector>

#define WM_LL_V 8        // int16 lanes of the reference's vector

static inline int16_t wm_ll_sat_add(int a, int b) { const int s = a + b; return (int16_t)(s > 32767 ? 32767 : s < -32768 ? -32768 : s); }
static inline int16_t wm_ll_usub(int16_t a, int16_t b) { const uint16_t x = (uint16_t)a, y = (uint16_t)b; return (int16_t)(x > y ? x - y : 0); }

// returns the score; *qe / *te = end coordinates (-1 / -1 for an empty target)
static inline int wm_ksw_ll_spec(int qlen, const uint8_t *query, int tlen, const uint8_t *target, const int8_t *mat, int gapo, int gape, int *qe, int *te)
{
	const int V = WM_LL_V, slen = (qlen + V - 1) / V, n = slen * V;
	std::vector<int16_t> profile((size_t)5 * n), Hprev(n, 0), Hcur(n, 0), E(n, 0), Hbest(n, 0);
	for (int a = 0; a < 5; ++a)                                     // ksw_ll_qinit, :32-78 (the int16 half)
		for (int j = 0; j < slen; ++j)
			for (int l = 0; l < V; ++l) {
				const int pos = j + l * slen;
				profile[((size_t)a * slen + j) * V + l] = pos < qlen ? mat[a * 5 + query[pos]] : 0;
			}
	const int16_t open_ext = (int16_t)(gapo + gape), ext = (int16_t)gape;
	int gmax = 0;
	*qe = *te = -1;
	for (int i = 0; i < tlen; ++i) {
		const int16_t *S = &profile[(size_t)target[i] * n];
		int16_t h[WM_LL_V], f[WM_LL_V], best[WM_LL_V];
		h[0] = 0;
		for (int l = 1; l < V; ++l) h[l] = Hprev[(size_t)(slen - 1) * V + l - 1];
		for (int l = 0; l < V; ++l) f[l] = 0, best[l] = 0;
		for (int j = 0; j < slen; ++j)                              // the main loop, :104-121
			for (int l = 0; l < V; ++l) {
				const size_t o = (size_t)j * V + l;
				int16_t e = E[o], v = wm_ll_sat_add(h[l], S[o]);
				v = v > e ? v : e; v = v > f[l] ? v : f[l];
				best[l] = best[l] > v ? best[l] : v;
				Hcur[o] = v;
				v = wm_ll_usub(v, open_ext);
				const int16_t e1 = wm_ll_usub(e, ext), f1 = wm_ll_usub(f[l], ext);
				E[o] = e1 > v ? e1 : v;
				f[l] = f1 > v ? f1 : v;
				h[l] = Hprev[o];
			}
		bool settled = false;
		for (int k = 0; k < V && !settled; ++k) {                  // lazy-F correction rounds, :122-133
			for (int l = V - 1; l > 0; --l) f[l] = f[l - 1];
			f[0] = 0;
			for (int j = 0; j < slen && !settled; ++j) {
				bool any = false;
				for (int l = 0; l < V; ++l) {
					const size_t o = (size_t)j * V + l;
					int16_t v = Hcur[o] > f[l] ? Hcur[o] : f[l];
					Hcur[o] = v;
					v = wm_ll_usub(v, open_ext);
					f[l] = wm_ll_usub(f[l], ext);
					any |= f[l] > v;
				}
				if (!any) settled = true;
			}
		}
		int imax = best[0];
		for (int l = 1; l < V; ++l) imax = imax > best[l] ? imax : best[l];
		if (imax >= gmax) { gmax = imax; *te = i; Hbest = Hcur; }   // :134-141
		Hprev.swap(Hcur);
	}
	for (int i = 0; i < n; ++i)                                     // :143-145
		if ((int)(uint16_t)Hbest[i] == gmax) *qe = i / V + i % V * slen;
	return gmax;
}

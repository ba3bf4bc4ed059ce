// cigar_fix.h — mm_fix_cigar (src/align.c:91-167) written ONCE as a literal loop over a plain array: left-align every indel that sits between two M ops,
// turn runs like 5I6D7I into one I and one D, squeeze out zero-length ops and merge equal neighbours (only if something asked for it), drop ONE leading I / D.
// The host mapper calls it (host/wm_align.cpp); it is the SPECIFICATION of the device form (fix_kernel.h behind wm_fix_extra_batch / wm_fix_extra_batch_pos),
// as wm_extra_walk (cigar_walk.h) is for the scan that follows. It carries no region: the caller applies  rev ? qe -= qshift : qs += qshift  and  rs += tshift.
// Sequences are 0..4 codes, one byte per base (the compare is on the codes: N equals N); CIGAR ops are BAM-encoded (len << 4 | op).
#pragma once
#include <stdint.h>

// cigar[0, *n_cigar) is rewritten in place, *n_cigar becomes the new count (never larger). qoff_end / toff_end (may be 0): the bases the raw CIGAR consumes, what the
// reference asserts against the region (:125). Returns 1 if the CIGAR or its count changed.
// A zero-length op of code >= 3 makes the reference index s[op] out of bounds (:132): callers must not pass one (the device entry points refuse it). A CIGAR whose ops
// all have length 0 leaves the reference reading cigar[0] of an empty CIGAR (:157); here it ends with *n_cigar = 0 and no shift.
static inline int wm_fix_cigar(uint32_t *cigar, int *n_cigar, const uint8_t *qseq, const uint8_t *tseq, int *qshift, int *tshift, int32_t *qoff_end, int32_t *toff_end)
{
	uint32_t n = (uint32_t)*n_cigar, k;
	int32_t toff = 0, qoff = 0, to_shrink = 0, moved = 0;
	*qshift = *tshift = 0;
	if (qoff_end) *qoff_end = 0;
	if (toff_end) *toff_end = 0;
	if (n <= 1) return 0;
	for (k = 0; k < n; ++k) {                                               // left-align indels
		const uint32_t op = cigar[k] & 0xf, len = cigar[k] >> 4;
		if (len == 0) to_shrink = 1;
		if (op == 0) toff += len, qoff += len;
		else if (op == 1 || op == 2) {
			if (k > 0 && k < n - 1 && (cigar[k - 1] & 0xf) == 0 && (cigar[k + 1] & 0xf) == 0) {
				int l;
				const int prev_len = cigar[k - 1] >> 4;
				if (op == 1) { for (l = 0; l < prev_len; ++l) if (qseq[qoff - 1 - l] != qseq[qoff + len - 1 - l]) break; }
				else { for (l = 0; l < prev_len; ++l) if (tseq[toff - 1 - l] != tseq[toff + len - 1 - l]) break; }
				if (l > 0) cigar[k - 1] -= (uint32_t)l << 4, cigar[k + 1] += (uint32_t)l << 4, qoff -= l, toff -= l, moved = 1;
				if (l == prev_len) to_shrink = 1;
			}
			if (op == 1) qoff += len; else toff += len;
		} else if (op == 3) toff += len;
	}
	if (qoff_end) *qoff_end = qoff;
	if (toff_end) *toff_end = toff;
	for (k = 0; k + 2 < n; ++k) {                                           // 5I6D7I -> one I and one D
		if ((cigar[k] & 0xf) > 0 && (cigar[k] & 0xf) + (cigar[k + 1] & 0xf) == 3) {
			uint32_t l, s[3] = { 0, 0, 0 };
			for (l = k; l < n; ++l) {
				const uint32_t op = cigar[l] & 0xf;
				if (op == 1 || op == 2 || cigar[l] >> 4 == 0) s[op] += cigar[l] >> 4;
				else break;
			}
			if (s[1] > 0 && s[2] > 0 && l - k > 2) {
				cigar[k] = s[1] << 4 | 1; cigar[k + 1] = s[2] << 4 | 2;
				for (k += 2; k < l; ++k) cigar[k] &= 0xf;
				to_shrink = 1;
			}
			k = l;
		}
	}
	if (to_shrink) {
		uint32_t l = 0;
		for (k = 0; k < n; ++k) if (cigar[k] >> 4 != 0) cigar[l++] = cigar[k];      // squeeze out zero-length ops
		n = l;
		for (k = l = 0; k < n; ++k)                                                 // merge equal neighbours
			if (k == n - 1 || (cigar[k] & 0xf) != (cigar[k + 1] & 0xf)) cigar[l++] = cigar[k];
			else cigar[k + 1] += cigar[k] >> 4 << 4;
		n = l;
	}
	int lead = 0;
	if (n > 0 && ((cigar[0] & 0xf) == 1 || (cigar[0] & 0xf) == 2)) {            // no leading I / D (one op only)
		const int32_t l = cigar[0] >> 4;
		if ((cigar[0] & 0xf) == 1) *qshift = l; else *tshift = l;
		--n; lead = 1;
		for (k = 0; k < n; ++k) cigar[k] = cigar[k + 1];
	}
	*n_cigar = (int)n;
	return moved || to_shrink || lead;
}

// cigar_eqx.h — mm_update_cigar_eqx (src/align.c:169-238), the tail of mm_update_extra under MM_F_EQX (:285), written ONCE as a literal loop over plain arrays: every
// M op of a FINAL CIGAR becomes its runs of '=' (code 7) and 'X' (code 8). The host mapper calls it (host/wm_align.cpp, host/wm_ops.cpp); it is the SPECIFICATION of the
// device form (eqx_kernel.h behind wm_eqx_batch / wm_eqx_batch_pos). Sequences are 0..4 codes, one byte per base, from the alignment's first base on (the caller has
// advanced them by mm_fix_cigar's shifts, :247); CIGAR ops are BAM-encoded (len << 4 | op).
//   * a run is a maximal stretch of columns of ONE M op with q == t, or with q != t. The compare is on the codes: N against N is '=' (the reference's TODO, :179);
//   * n_EQX = runs over the whole CIGAR, n_M = ops of code 0 — a zero-length M op counts in n_M and has no run (:178, :185);
//   * only codes 0..3 advance the operands (:186-192); every op of another code is copied as it stands, zero lengths included (:233).
#pragma once
#include <stdint.h>

// number of runs (n_EQX) of cigar[0, n); *n_M = ops of code 0 (src/align.c:175-193)
static inline uint32_t wm_cigar_eqx_count(const uint32_t *cigar, int n, const uint8_t *qseq, const uint8_t *tseq, uint32_t *n_M)
{
	uint32_t n_EQX = 0, k, l, toff = 0, qoff = 0;
	*n_M = 0;
	for (k = 0; k < (uint32_t)n; ++k) {
		uint32_t op = cigar[k] & 0xf, len = cigar[k] >> 4;
		if (op == 0) {
			while (len > 0) {
				for (l = 0; l < len && qseq[qoff + l] == tseq[toff + l]; ++l) {}      // run of '='
				if (l > 0) { ++n_EQX; len -= l; toff += l; qoff += l; }
				for (l = 0; l < len && qseq[qoff + l] != tseq[toff + l]; ++l) {}      // run of 'X'
				if (l > 0) { ++n_EQX; len -= l; toff += l; qoff += l; }
			}
			++*n_M;
		} else if (op == 1) qoff += len;
		else if (op == 2 || op == 3) toff += len;
	}
	return n_EQX;
}

// the two branches on their own, for a caller that has counted (host/wm_ops.cpp sizes its output first): src/align.c:195-201 ...
static inline int wm_cigar_eqx_relabel(const uint32_t *cigar, int n, uint32_t *out)
{
	for (int k = 0; k < n; ++k) out[k] = (cigar[k] & 0xf) == 0 ? cigar[k] >> 4 << 4 | 7 : cigar[k];
	return n;
}
// ... and :209-234
static inline int wm_cigar_eqx_rewrite(const uint32_t *cigar, int n, const uint8_t *qseq, const uint8_t *tseq, uint32_t *out)
{
	uint32_t k, l, m = 0, toff = 0, qoff = 0;
	for (k = 0; k < (uint32_t)n; ++k) {
		uint32_t op = cigar[k] & 0xf, len = cigar[k] >> 4;
		if (op == 0) {
			while (len > 0) {
				for (l = 0; l < len && qseq[qoff + l] == tseq[toff + l]; ++l) {}
				if (l > 0) out[m++] = l << 4 | 7;
				len -= l; toff += l; qoff += l;
				for (l = 0; l < len && qseq[qoff + l] != tseq[toff + l]; ++l) {}
				if (l > 0) out[m++] = l << 4 | 8;
				len -= l; toff += l; qoff += l;
			}
			continue;
		} else if (op == 1) qoff += len;
		else if (op == 2 || op == 3) toff += len;
		out[m++] = cigar[k];
	}
	return (int)m;
}
// cigar[0, n) -> out[0, return value); out must hold  n - n_M + n_EQX  ops (never more than n + the M columns; out == cigar is fine when *in_place comes back 1, and
// wm_cigar_eqx_count tells beforehand). *in_place: which of the reference's two branches ran.
// THE QUIRK (src/align.c:195-201): if n_EQX == n_M the reference relabels every M op as '=' WITHOUT looking at its bases again. One run per M op is what an all-match
// CIGAR has — but also one whose M op is entirely mismatches (10M1I1M1D10M with the middle base differing gives 10=1I1=1D10=), and a zero-length M op (no run) balances
// an M op with two runs elsewhere. That is the reference's output, so it is reproduced here.
static inline int wm_cigar_eqx(const uint32_t *cigar, int n, const uint8_t *qseq, const uint8_t *tseq, uint32_t *out, int *in_place)
{
	uint32_t n_M;
	const uint32_t n_EQX = wm_cigar_eqx_count(cigar, n, qseq, tseq, &n_M);
	*in_place = n_EQX == n_M;
	return n_EQX == n_M ? wm_cigar_eqx_relabel(cigar, n, out) : wm_cigar_eqx_rewrite(cigar, n, qseq, tseq, out);
}

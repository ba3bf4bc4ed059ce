// cigar_cs.h — write_cs_core and write_MD_core (src/format.c:141-187, :189-218), the bodies of the cs:Z / MD:Z tags under --cs, --cs=long and --MD, written ONCE as a
// literal loop over plain arrays. The host formatter calls it (host/wm_format.cpp keeps the operand preparation of write_cs_or_MD, :220-243, and the "\tcs:Z:" /
// "\tMD:Z:" prefix); it is the SPECIFICATION of the device form (cs_kernel.h behind wm_cs_batch / wm_cs_batch_pos). Sequences are 0..4 codes, one byte per base, from
// the alignment's first base on, as in cigar_eqx.h; CIGAR ops are BAM-encoded (len << 4 | op). Only the tag's BODY is written, no terminator.
//   * the CODES are compared (:151, :198): N against N is a match — MD counts it, cs long prints 'N'. THE CONTRACT IS CODES 0..4; a byte above 4 is clamped to 4
//     before it is compared or printed, so "acgtn"[c] is never read out of range (the reference would read past its table);
//   * op codes 7 and 8 are treated like 0 (:148, :196): the bases decide, not the code. An op code outside {0, 1, 2, 3, 7, 8} (the assert of :147 / :195) and, in a
//     cs mode, an N op shorter than 2 (the assert of :180) are ERRORS: wm_cigar_cs_check names the op, wm_cigar_cs writes nothing for such a CIGAR;
//   * cs (:145-185): the identical run belongs to ONE op of code 0 / 7 / 8 (l_tmp starts at 0 in every op, :149). It is flushed as ":<n>" (short) or "=<BASES>" (long,
//     upper case, :160) before a mismatch (:152-158) and at the op's end (:162-167); a run of 0 prints nothing — so 10M10M without a mismatch is ":10:10". A mismatch
//     is "*<t><q>" in lower case (:159). I is "+<bases>", D is "-<bases>", lower case, and a zero-length I / D the bare sign (:169-178). N is
//     "~<t0><t1><len><t[len-2]><t[len-1]>" (:181-182);
//   * MD (:191-216): ONE run counter l_MD for the whole CIGAR; it passes through I and N ops (:204-205, :212-213) and across op boundaries. A mismatch prints
//     "<run><T>" (upper case) and resets the run, "0" included when the run is 0 (:199-200). D prints "<run>^<BASES>" and resets it; a zero-length D prints "<run>^"
//     (:207-210). The final run is printed only if it is > 0 (:216). An empty CIGAR gives an empty body.
#pragma once
#include <stdint.h>

#define WM_CS_SHORT 0       /* --cs        (no_iden = 1) */
#define WM_CS_LONG  1       /* --cs=long   (no_iden = 0) */
#define WM_CS_MD    2       /* --MD */

// decimal digits of v at o; returns their number
static inline int wm_cs_put_uint(char *o, uint32_t v)
{
	char b[10];
	int n = 0, i;
	do { b[n++] = (char)('0' + v % 10); v /= 10; } while (v);
	for (i = 0; i < n; ++i) o[i] = b[n - 1 - i];
	return n;
}

// the first op the reference asserts against (:147, :180, :195), or -1; mode outside 0..2: -2
static inline int wm_cigar_cs_check(int mode, const uint32_t *cigar, int n)
{
	if (mode < WM_CS_SHORT || mode > WM_CS_MD) return -2;
	for (int k = 0; k < n; ++k) {
		const uint32_t op = cigar[k] & 0xf, len = cigar[k] >> 4;
		if (!(op <= 3 || op == 7 || op == 8)) return k;
		if (op == 3 && mode != WM_CS_MD && len < 2) return k;
	}
	return -1;
}

// bytes no body of this CIGAR exceeds, in any mode: 3 per column of an M op ("*tq"; a run's ":<n>" or "=<BASES>" is at most 2 per column) and a sign or a run of
// 10 digits per op, 1 per gap base, "~tt<len>tt" per intron
static inline int64_t wm_cigar_cs_bound(const uint32_t *cigar, int n)
{
	int64_t b = 11;
	for (int k = 0; k < n; ++k) {
		const uint32_t op = cigar[k] & 0xf;
		const int64_t len = cigar[k] >> 4;
		b += op == 1 || op == 2 ? len + 12 : op == 3 ? 16 : 3 * len + 12;
	}
	return b;
}

// cigar[0, n) over qseq / tseq -> the body at out (room for wm_cigar_cs_bound bytes is always enough); returns the bytes written, or -(k + 1) for the op k that
// wm_cigar_cs_check names (-(n + 1) for a bad mode)
static inline int64_t wm_cigar_cs(int mode, const uint32_t *cigar, int n, const uint8_t *qseq, const uint8_t *tseq, char *out)
{
	static const char lower[] = "acgtn", upper[] = "ACGTN";
	const int bad = wm_cigar_cs_check(mode, cigar, n);
	if (bad != -1) return bad == -2 ? -((int64_t)n + 1) : -((int64_t)bad + 1);
	char *o = out;
	uint32_t q_off = 0, t_off = 0, j;
#define WM_CS_CODE(s, i) ((s)[i] > 4 ? 4 : (s)[i])
	if (mode == WM_CS_MD) {
		uint32_t l_MD = 0;
		for (int k = 0; k < n; ++k) {
			const uint32_t op = cigar[k] & 0xf, len = cigar[k] >> 4;
			if (op == 0 || op == 7 || op == 8) {
				for (j = 0; j < len; ++j) {
					const int qc = WM_CS_CODE(qseq, q_off + j), tc = WM_CS_CODE(tseq, t_off + j);
					if (qc != tc) { o += wm_cs_put_uint(o, l_MD); *o++ = upper[tc]; l_MD = 0; }
					else ++l_MD;
				}
				q_off += len; t_off += len;
			} else if (op == 1) q_off += len;
			else if (op == 2) {
				o += wm_cs_put_uint(o, l_MD); *o++ = '^';
				for (j = 0; j < len; ++j) *o++ = upper[WM_CS_CODE(tseq, t_off + j)];
				l_MD = 0; t_off += len;
			} else t_off += len;
		}
		if (l_MD > 0) o += wm_cs_put_uint(o, l_MD);
		return o - out;
	}
	for (int k = 0; k < n; ++k) {
		const uint32_t op = cigar[k] & 0xf, len = cigar[k] >> 4;
		if (op == 0 || op == 7 || op == 8) {
			uint32_t l_tmp = 0;
			for (j = 0; j <= len; ++j) {                       // j == len: the flush at the op's end
				int qc = 0, tc = 1;
				if (j < len) { qc = WM_CS_CODE(qseq, q_off + j); tc = WM_CS_CODE(tseq, t_off + j); }
				if (qc == tc) { ++l_tmp; continue; }
				if (l_tmp > 0) {
					if (mode == WM_CS_LONG) { *o++ = '='; for (uint32_t i = j - l_tmp; i < j; ++i) *o++ = upper[WM_CS_CODE(qseq, q_off + i)]; }
					else { *o++ = ':'; o += wm_cs_put_uint(o, l_tmp); }
					l_tmp = 0;
				}
				if (j < len) { *o++ = '*'; *o++ = lower[tc]; *o++ = lower[qc]; }
			}
			q_off += len; t_off += len;
		} else if (op == 1) {
			*o++ = '+';
			for (j = 0; j < len; ++j) *o++ = lower[WM_CS_CODE(qseq, q_off + j)];
			q_off += len;
		} else if (op == 2) {
			*o++ = '-';
			for (j = 0; j < len; ++j) *o++ = lower[WM_CS_CODE(tseq, t_off + j)];
			t_off += len;
		} else {
			*o++ = '~'; *o++ = lower[WM_CS_CODE(tseq, t_off)]; *o++ = lower[WM_CS_CODE(tseq, t_off + 1)];
			o += wm_cs_put_uint(o, len);
			*o++ = lower[WM_CS_CODE(tseq, t_off + len - 2)]; *o++ = lower[WM_CS_CODE(tseq, t_off + len - 1)];
			t_off += len;
		}
	}
#undef WM_CS_CODE
	return o - out;
}

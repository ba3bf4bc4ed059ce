// tests/simt_emu/emu_fix_main.cpp — TEST INFRASTRUCTURE ONLY.
// A stand-alone driver of emu_fix.cpp for sanitizer builds (-fsanitize=address,undefined): it reads the cases `python tests/fixcases.py dump FILE` wrote, runs each
// through the specification and through the emulated kernels — byte form and position form, the fix alone and fused with the scan at a short and a long routing — and compares CIGAR,
// count, both shifts and `changed`. The index arithmetic off - 1 - j of pass 1 is where this code would read out of bounds; every job gets buffers of exactly its
// size, so the sanitizer sees such a read. Exit status 0 = all equal and nothing reported.
// File: int32 n_cases, then per case: int32 score[5], n_cigar, qlen, tlen; uint32 cigar[n_cigar]; uint8 q[qlen]; uint8 t[tlen]  (lengths include the padding).
#include <stdint.h>
#include <stdio.h>
#include <string.h>
#include <vector>

extern "C" {
void emu_fix_spec(uint32_t *cig, int n, const uint8_t *q, const uint8_t *t, int32_t *out4);
int emu_fix_batch(int n_jobs, const int32_t *score5, const uint32_t *q_off, const uint32_t *t_off, const uint32_t *cig_off, const int32_t *n_cigar,
                  const uint8_t *seqs, size_t seqs_bytes, const uint32_t *cigars, uint32_t *cigars_out, int long_min_cols, int tile_cols, int32_t *fix4, int32_t *out6);
int emu_fix_batch_pos(int n_jobs, const int32_t *score5, const int64_t *qwin_off, const int32_t *qwin_len, const int32_t *q_pos, const int64_t *t_base,
                      const uint32_t *cig_off, const int32_t *n_cigar, const uint8_t *reads, size_t n_reads, const uint8_t *ref, size_t n_ref,
                      const uint32_t *cigars, uint32_t *cigars_out, int long_min_cols, int tile_cols, int32_t *fix4, int32_t *out6);
}

int main(int argc, char **argv)
{
	if (argc < 2) { fprintf(stderr, "usage: %s cases.bin\n", argv[0]); return 2; }
	FILE *f = fopen(argv[1], "rb");
	if (!f) { perror(argv[1]); return 2; }
	int32_t n_cases = 0, bad = 0;
	if (fread(&n_cases, 4, 1, f) != 1) return 2;
	for (int i = 0; i < n_cases; ++i) {
		int32_t h[8];
		if (fread(h, 4, 8, f) != 8) return 2;
		const int n = h[5], ql = h[6], tl = h[7];
		std::vector<uint32_t> cig((size_t)n), out((size_t)n), want((size_t)n);
		std::vector<uint8_t> seqs((size_t)ql + tl);
		if ((n && fread(cig.data(), 4, n, f) != (size_t)n) || (ql + tl && fread(seqs.data(), 1, (size_t)ql + tl, f) != (size_t)(ql + tl))) return 2;
		want = cig;
		int32_t w4[4];
		emu_fix_spec(want.data(), n, seqs.data(), seqs.data() + ql, w4);
		// (the query first, then the target first: each operand once at the very start of the buffer, where a read in front of it leaves the allocation)
		std::vector<uint8_t> swapped(seqs.begin() + ql, seqs.end());
		swapped.insert(swapped.end(), seqs.begin(), seqs.begin() + ql);
		const uint32_t cig_off = 0;
		const int routes[3][2] = { { 1 << 30, 512 }, { 1 << 30, 512 }, { 1, 64 } };
		for (int r = 0; r < 6; ++r) {
			int32_t f4[4], x6[6];
			const bool t_first = r >= 3;
			const uint32_t q_off = t_first ? (uint32_t)tl : 0, t_off = t_first ? 0 : (uint32_t)ql;
			const std::vector<uint8_t> &sq = t_first ? swapped : seqs;
			std::fill(out.begin(), out.end(), 0xdeadbeefu);
			emu_fix_batch(1, r % 3 ? h : 0, &q_off, &t_off, &cig_off, &n, sq.data(), sq.size(), cig.data(), out.data(), routes[r % 3][0], routes[r % 3][1], f4, x6);
			if (memcmp(f4, w4, sizeof(f4)) || (w4[0] > 0 && memcmp(out.data(), want.data(), (size_t)w4[0] * 4))) { fprintf(stderr, "case %d route %d differs\n", i, r); ++bad; }
		}
		// the position form: the query as a resident read of exactly ql bases (forward strand from its first base), the target as a reference of exactly tl bases —
		// packed words and nibbles of exactly that size
		for (int r = 0; r < 3; ++r) {
			int32_t f4[4], x6[6];
			const int64_t qwin = 0, t_base = 0;
			const int32_t qlen = ql, q_pos = 0;
			std::fill(out.begin(), out.end(), 0xdeadbeefu);
			emu_fix_batch_pos(1, r ? h : 0, &qwin, &qlen, &q_pos, &t_base, &cig_off, &n, seqs.data(), (size_t)ql, seqs.data() + ql, (size_t)tl, cig.data(), out.data(),
			                  routes[r][0], routes[r][1], f4, x6);
			if (memcmp(f4, w4, sizeof(f4)) || (w4[0] > 0 && memcmp(out.data(), want.data(), (size_t)w4[0] * 4))) { fprintf(stderr, "case %d position route %d differs\n", i, r); ++bad; }
		}
	}
	fclose(f);
	printf("%d cases, %d differ\n", n_cases, bad);
	return bad ? 1 : 0;
}

// tests/simt_emu/emu_fix.cpp — TEST INFRASTRUCTURE ONLY.
// mm_fix_cigar on the host wavefront emulator (winnowmap_amd/csrc/fix_kernel.h), alone or fused with the fold of mm_update_extra's scan (extra_kernel.h) the way
// csrc/wm_extra.hip launches them: prefix pass over the RAW CIGAR, the fix into a second pool, prefix pass over the fixed CIGAR with the operands advanced by both
// shifts, then either class — chosen, and its tiles counted, from the RAW CIGAR. Byte form and position form. emu_fix_spec is the specification itself (cigar_fix.h).
#include <stdint.h>
#include "simt.h"                    // the emulator (this directory is first on the include path)
#include "fix_kernel.h"              // winnowmap_amd/csrc
#include "cigar_fix.h"
#include <vector>
#include <string.h>

namespace {
wmk::extra_src_bytes advance(wmk::extra_src_bytes S, int qshift, int tshift) { S.qb += qshift; S.tb += tshift; return S; }
wmk::extra_src_pos advance(wmk::extra_src_pos S, int qshift, int tshift) { S.q_pos += qshift; S.tb += tshift; return S; }

template <class MakeSrc>
void run_jobs(int n_jobs, const int32_t *score5, const uint32_t *cig_off, const int32_t *n_cigar, const uint32_t *cigars, uint32_t *cigars_out, int long_min_cols,
              int tile_cols, int32_t *fix4, int32_t *out6, const MakeSrc &make)
{
	for (int j = 0; j < n_jobs; ++j) {
		const int n = n_cigar[j];
		const uint32_t *cig = cigars + cig_off[j];
		uint32_t *fixed = cigars_out + cig_off[j];
		std::vector<int> c(n + 1, 0x5a5a5a5a), q(n + 1, 0x5a5a5a5a), t(n + 1, 0x5a5a5a5a);          // poisoned scratch: a slot the kernels should not read shows
		simt::exec_mask() = ~0ull;
		wmk::extra_prefix(cig, n, c.data(), q.data(), t.data());
		const int raw_cols = c[n];
		const auto S = make(j);
		int32_t *fr = fix4 + (size_t)j * 4;
		fr[0] = fr[1] = fr[2] = fr[3] = -1;
		wmk::fix_cigar_wave(S, cig, n, q.data(), t.data(), c.data(), fixed, fr);
		if (!score5) continue;
		const wm_extra_score_t sc = { score5[0], score5[1], score5[2], score5[3], score5[4] };
		const auto S2 = advance(S, fr[1], fr[2]);
		const int n2 = fr[0];
		std::fill(c.begin(), c.end(), 0x5a5a5a5a); std::fill(q.begin(), q.end(), 0x5a5a5a5a); std::fill(t.begin(), t.end(), 0x5a5a5a5a);
		wmk::extra_prefix(fixed, n2, c.data(), q.data(), t.data());
		int32_t res[6] = { -1, -1, -1, -1, -1, -1 };
		if (raw_cols <= 0 || raw_cols < long_min_cols) wmk::extra_short(S2, sc, fixed, c.data(), q.data(), t.data(), n2, tile_cols, res);
		else {
			const int n_tiles = (raw_cols + tile_cols - 1) / tile_cols;                               // (the raw count: surplus tiles contribute the identity)
			std::vector<int> part((size_t)n_tiles * 8, 0x5a5a5a5a);
			for (int tile = n_tiles - 1; tile >= 0; --tile)
				wmk::extra_long_tile(S2, sc, fixed, c.data(), q.data(), t.data(), n2, tile_cols, tile, part.data() + (size_t)tile * 8);
			wmk::extra_combine(part.data(), n_tiles, q.data(), t.data(), n2, res);
		}
		memcpy(out6 + (size_t)j * 6, res, sizeof(res));
	}
}
} // namespace

extern "C" {

// the specification: cig[0, n) in place -> out4 = { n_cigar, qshift, tshift, changed }
void emu_fix_spec(uint32_t *cig, int n, const uint8_t *q, const uint8_t *t, int32_t *out4)
{
	int qs = 0, ts = 0, nn = n;
	const int ch = wm_fix_cigar(cig, &nn, q, t, &qs, &ts, 0, 0);
	out4[0] = nn; out4[1] = qs; out4[2] = ts; out4[3] = ch;
}

// byte form: operands at seqs + q_off[j] / t_off[j]. score5 == NULL: the fix alone
int emu_fix_batch(int n_jobs, const int32_t *score5, const uint32_t *q_off, const uint32_t *t_off, const uint32_t *cig_off, const int32_t *n_cigar,
                  const uint8_t *seqs, size_t seqs_bytes, const uint32_t *cigars, uint32_t *cigars_out, int long_min_cols, int tile_cols, int32_t *fix4, int32_t *out6)
{
	std::vector<uint64_t> slab(seqs_bytes / 8 + 2, 0x0909090909090909ULL);          // 8-byte aligned, the word behind the last base readable (poisoned)
	memcpy(slab.data(), seqs, seqs_bytes);
	const uint8_t *sq = (const uint8_t*)slab.data();
	run_jobs(n_jobs, score5, cig_off, n_cigar, cigars, cigars_out, long_min_cols, tile_cols, fix4, out6,
	         [&](int j) { wmk::extra_src_bytes S = { sq, (long long)q_off[j], (long long)t_off[j] }; return S; });
	return 0;
}

// position form: reads = 0..4 codes of the resident reads (packed here), ref = 0..15 codes of the reference, one per base (packed to nibbles here)
int emu_fix_batch_pos(int n_jobs, const int32_t *score5, const int64_t *qwin_off, const int32_t *qwin_len, const int32_t *q_pos, const int64_t *t_base,
                      const uint32_t *cig_off, const int32_t *n_cigar, const uint8_t *reads, size_t n_reads, const uint8_t *ref, size_t n_ref,
                      const uint32_t *cigars, uint32_t *cigars_out, int long_min_cols, int tile_cols, int32_t *fix4, int32_t *out6)
{
	std::vector<uint64_t> pk(wm_pk_words(n_reads), 0), nm(wm_nm_words(n_reads), 0);
	wm_pack_codes(reads, n_reads, pk.data(), nm.data());
	std::vector<uint32_t> S(n_ref / 8 + 2, 0x99999999u);
	for (size_t i = 0; i < n_ref; ++i) S[i >> 3] = (S[i >> 3] & ~(0xfu << ((i & 7) << 2))) | ((uint32_t)(ref[i] & 0xf) << ((i & 7) << 2));
	run_jobs(n_jobs, score5, cig_off, n_cigar, cigars, cigars_out, long_min_cols, tile_cols, fix4, out6,
	         [&](int j) { wmk::extra_src_pos P = { pk.data(), nm.data(), S.data(), (long long)qwin_off[j], (long long)t_base[j], q_pos[j], qwin_len[j] }; return P; });
	return 0;
}

} // extern "C"

// tests/simt_emu/emu_extra.cpp — TEST INFRASTRUCTURE ONLY.
// The fold of mm_update_extra's scan (winnowmap_amd/csrc/extra_kernel.h) on the host wavefront emulator: the prefix pass, then either class — one wavefront
// walking a job's tiles, or one wavefront per tile plus the combine pass — over the byte form and over the position form (reads packed with wm_pack_codes,
// the target as 4-bit nibbles like the S array of the index). The planning mirrors csrc/wm_extra.hip: the class is chosen by long_min_cols, results must not depend on it.
#include <stdint.h>
#include "simt.h"                    // the emulator (this directory is first on the include path)
#include "extra_kernel.h"            // winnowmap_amd/csrc
#include <vector>
#include <string.h>

namespace {
template <class MakeSrc>
void run_jobs(int n_jobs, const wm_extra_score_t &sc, const uint32_t *cig_off, const int32_t *n_cigar, const uint32_t *cigars, size_t n_ops, int long_min_cols,
              int tile_cols, int32_t *out6, int32_t *n_long, const MakeSrc &make)
{
	// poisoned scratch: a slot the kernels should not read shows
	size_t n_pre = 0, pre = 0;
	for (int j = 0; j < n_jobs; ++j) n_pre += (size_t)n_cigar[j] + 1;
	(void)n_ops;
	std::vector<int> colS(n_pre, 0x5a5a5a5a), qS(n_pre, 0x5a5a5a5a), tS(n_pre, 0x5a5a5a5a);
	*n_long = 0;
	for (int j = 0; j < n_jobs; pre += (size_t)n_cigar[j] + 1, ++j) {
		const uint32_t *cig = cigars + cig_off[j];
		int *c = colS.data() + pre, *q = qS.data() + pre, *t = tS.data() + pre;
		simt::exec_mask() = ~0ull;
		wmk::extra_prefix(cig, n_cigar[j], c, q, t);
		const int ncols = c[n_cigar[j]];
		const auto S = make(j);
		int32_t res[6] = { -1, -1, -1, -1, -1, -1 };
		if (ncols < long_min_cols) wmk::extra_short(S, sc, cig, c, q, t, n_cigar[j], tile_cols, res);
		else {
			const int n_tiles = (ncols + tile_cols - 1) / tile_cols;
			std::vector<int> part((size_t)n_tiles * 8, 0x5a5a5a5a);
			for (int tile = n_tiles - 1; tile >= 0; --tile)          // (any order: the tiles are independent wavefronts)
				wmk::extra_long_tile(S, sc, cig, c, q, t, n_cigar[j], tile_cols, tile, part.data() + (size_t)tile * 8);
			wmk::extra_combine(part.data(), n_tiles, q, t, n_cigar[j], res);
			++*n_long;
		}
		memcpy(out6 + (size_t)j * 6, res, sizeof(res));
	}
}
} // namespace

extern "C" {

// the four-line composition as the kernels compile it (uniform form)
void emu_extra_compose(const int32_t *L, const int32_t *R, int32_t *out)
{
	int l[4] = { L[0], L[1], L[2], L[3] };
	const int r[4] = { R[0], R[1], R[2], R[3] };
	wmk::extra_compose(l, r);
	for (int i = 0; i < 4; ++i) out[i] = l[i];
}
// ... and the ordered wave reduction over 64 tuples (tuples[64][4] -> out[4])
void emu_extra_wave_fold(const int32_t *tuples, int32_t *out)
{
	simt::exec_mask() = ~0ull;
	simt::V<int> a, b, m, c;
	for (int i = 0; i < 64; ++i) { a.v[i] = tuples[4 * i]; b.v[i] = tuples[4 * i + 1]; m.v[i] = tuples[4 * i + 2]; c.v[i] = tuples[4 * i + 3]; }
	wmk::extra_wave_fold(a, b, m, c);
	out[0] = a.v[0]; out[1] = b.v[0]; out[2] = m.v[0]; out[3] = c.v[0];
}

// byte form: operands at seqs + q_off[j] / t_off[j]
int emu_extra_batch(int n_jobs, const int32_t *score5, const uint32_t *q_off, const uint32_t *t_off, const uint32_t *cig_off, const int32_t *n_cigar,
                    const uint8_t *seqs, size_t seqs_bytes, const uint32_t *cigars, size_t n_ops, int long_min_cols, int tile_cols, int32_t *out6, int32_t *n_long)
{
	const wm_extra_score_t sc = { score5[0], score5[1], score5[2], score5[3], score5[4] };
	std::vector<uint64_t> slab(seqs_bytes / 8 + 2, 0x0909090909090909ULL);          // 8-byte aligned, the word behind the last base readable (poisoned)
	memcpy(slab.data(), seqs, seqs_bytes);
	const uint8_t *sq = (const uint8_t*)slab.data();
	run_jobs(n_jobs, sc, cig_off, n_cigar, cigars, n_ops, long_min_cols, tile_cols, out6, n_long,
	         [&](int j) { wmk::extra_src_bytes S = { sq, (long long)q_off[j], (long long)t_off[j] }; return S; });
	return 0;
}

// position form: reads = 0..4 codes of the resident reads (packed here), ref = 0..15 codes of the reference, one per base (packed to nibbles here);
// t_base[j] = index of the job's first target base in ref
int emu_extra_batch_pos(int n_jobs, const int32_t *score5, const int64_t *qwin_off, const int32_t *qwin_len, const int32_t *q_pos, const int64_t *t_base,
                        const uint32_t *cig_off, const int32_t *n_cigar, const uint8_t *reads, size_t n_reads, const uint8_t *ref, size_t n_ref,
                        const uint32_t *cigars, size_t n_ops, int long_min_cols, int tile_cols, int32_t *out6, int32_t *n_long)
{
	const wm_extra_score_t sc = { score5[0], score5[1], score5[2], score5[3], score5[4] };
	std::vector<uint64_t> pk(wm_pk_words(n_reads), 0), nm(wm_nm_words(n_reads), 0);
	wm_pack_codes(reads, n_reads, pk.data(), nm.data());
	std::vector<uint32_t> S(n_ref / 8 + 2, 0x99999999u);
	for (size_t i = 0; i < n_ref; ++i) S[i >> 3] = (S[i >> 3] & ~(0xfu << ((i & 7) << 2))) | ((uint32_t)(ref[i] & 0xf) << ((i & 7) << 2));
	run_jobs(n_jobs, sc, cig_off, n_cigar, cigars, n_ops, long_min_cols, tile_cols, out6, n_long,
	         [&](int j) { wmk::extra_src_pos P = { pk.data(), nm.data(), S.data(), (long long)qwin_off[j], (long long)t_base[j], q_pos[j], qwin_len[j] }; return P; });
	return 0;
}

} // extern "C"

// tests/simt_emu/emu_eqx.cpp — TEST INFRASTRUCTURE ONLY.
// mm_update_cigar_eqx on the host wavefront emulator (winnowmap_amd/csrc/eqx_kernel.h), launched the way csrc/wm_eqx.hip launches it: prefix pass, the count pass in
// either class, the scan over jobs, the write pass of the jobs in the rewrite branch, the ops pass of every job. Byte form and position form. emu_eqx_spec is the
// specification itself (cigar_eqx.h).
#include <stdint.h>
#include "simt.h"                    // the emulator (this directory is first on the include path)
#include "eqx_kernel.h"              // winnowmap_amd/csrc
#include "cigar_eqx.h"
#include <vector>
#include <string.h>

namespace {
const int POISON = 0x5a5a5a5a;
struct Pre { std::vector<int> m, q, t, c, g; };

template <class MakeSrc>
int run_jobs(int n_jobs, const uint32_t *cig_off, const int32_t *n_cigar, const uint32_t *cigars, int long_min_cols, int tile_cols, uint32_t *out, size_t out_cap,
             int32_t *res4, const MakeSrc &make)
{
	std::vector<Pre> pre(n_jobs);
	std::vector<std::vector<int>> part(n_jobs);
	std::vector<int> cnt((size_t)n_jobs * 3 + 1, POISON);
	auto is_long = [&](int j) { const int cols = pre[j].m[n_cigar[j]]; return cols > 0 && cols >= long_min_cols; };
	for (int j = 0; j < n_jobs; ++j) {                                       // prefix + count
		const int n = n_cigar[j];
		const uint32_t *cig = cigars + cig_off[j];
		Pre &P = pre[j];
		P.m.assign(n + 1, POISON); P.q.assign(n + 1, POISON); P.t.assign(n + 1, POISON); P.c.assign(n + 1, POISON); P.g.assign(n + 1, POISON);      // a slot the kernels should not read shows
		simt::exec_mask() = ~0ull;
		wmk::eqx_prefix(cig, n, P.m.data(), P.q.data(), P.t.data(), P.c.data(), P.g.data());
		const auto S = make(j);
		if (!is_long(j)) wmk::eqx_short_count(S, cig, P.m.data(), P.q.data(), P.t.data(), P.c.data(), n, tile_cols, cnt.data() + (size_t)j * 3);
		else {
			const int n_tiles = (P.m[n] + tile_cols - 1) / tile_cols;
			part[j].assign((size_t)n_tiles * 2, POISON);
			for (int tile = n_tiles - 1; tile >= 0; --tile)
				wmk::eqx_long_count(S, cig, P.m.data(), P.q.data(), P.t.data(), P.c.data(), n, tile_cols, tile, part[j].data() + (size_t)tile * 2);
			wmk::eqx_combine(part[j].data(), n_tiles, P.c.data(), n, cnt.data() + (size_t)j * 3);
		}
	}
	int total = POISON;
	wmk::eqx_job_scan(cnt.data(), n_jobs, res4, &total);
	if ((size_t)total > out_cap) return total;
	std::vector<uint32_t> pool((size_t)total + 1, 0xdeadbeefu);                // exactly the reported size, a guard word behind it
	for (int j = 0; j < n_jobs; ++j) {                                       // write
		const int n = n_cigar[j];
		const uint32_t *cig = cigars + cig_off[j];
		Pre &P = pre[j];
		uint32_t *o = pool.data() + res4[(size_t)j * 4];
		const int in_place = res4[(size_t)j * 4 + 3];
		if (!in_place) {
			const auto S = make(j);
			if (!is_long(j)) wmk::eqx_short_write(S, cig, P.m.data(), P.q.data(), P.t.data(), P.c.data(), n, tile_cols, o, P.g.data());
			else
				for (int tile = (int)part[j].size() / 2 - 1; tile >= 0; --tile)
					wmk::eqx_long_write(S, cig, P.m.data(), P.q.data(), P.t.data(), P.c.data(), n, tile_cols, tile, part[j].data() + (size_t)tile * 2, o, P.g.data());
		}
		wmk::eqx_ops_write(cig, n, P.c.data(), P.g.data(), in_place, o);
	}
	if (pool[total] != 0xdeadbeefu) return -1;                                // a store behind the call's output
	for (int i = 0; i < total; ++i) if (pool[i] == 0xdeadbeefu) return -2;     // a slot nobody wrote (no real op has this word: code 15)
	memcpy(out, pool.data(), (size_t)total * 4);
	return total;
}
} // namespace

extern "C" {

// the specification: cig[0, n) -> out (room for n + M columns ops); returns the new count, *in_place the branch
int emu_eqx_spec(const uint32_t *cig, int n, const uint8_t *q, const uint8_t *t, uint32_t *out, int32_t *in_place)
{
	int ip = 0;
	const int m = wm_cigar_eqx(cig, n, q, t, out, &ip);
	*in_place = ip;
	return m;
}

// byte form: operands at seqs + q_off[j] / t_off[j]. Returns the ops of the whole call (> out_cap: nothing written), res4 = wm_eqx_res_t per job; < 0: see run_jobs
int emu_eqx_batch(int n_jobs, const uint32_t *q_off, const uint32_t *t_off, const uint32_t *cig_off, const int32_t *n_cigar, const uint8_t *seqs, size_t seqs_bytes,
                  const uint32_t *cigars, int long_min_cols, int tile_cols, uint32_t *out, size_t out_cap, int32_t *res4)
{
	std::vector<uint64_t> slab(seqs_bytes / 8 + 2, 0x0909090909090909ULL);
	memcpy(slab.data(), seqs, seqs_bytes);
	const uint8_t *sq = (const uint8_t*)slab.data();
	return run_jobs(n_jobs, cig_off, n_cigar, cigars, long_min_cols, tile_cols, out, out_cap, res4,
	                [&](int j) { wmk::extra_src_bytes S = { sq, (long long)q_off[j], (long long)t_off[j] }; return S; });
}

// position form: reads = 0..4 codes of the resident reads (packed here), ref = 0..15 codes of the reference, one per base (packed to nibbles here)
int emu_eqx_batch_pos(int n_jobs, const int64_t *qwin_off, const int32_t *qwin_len, const int32_t *q_pos, const int64_t *t_base, const uint32_t *cig_off,
                      const int32_t *n_cigar, const uint8_t *reads, size_t n_reads, const uint8_t *ref, size_t n_ref, const uint32_t *cigars, int long_min_cols,
                      int tile_cols, uint32_t *out, size_t out_cap, int32_t *res4)
{
	std::vector<uint64_t> pk(wm_pk_words(n_reads), 0), nm(wm_nm_words(n_reads), 0);
	wm_pack_codes(reads, n_reads, pk.data(), nm.data());
	std::vector<uint32_t> S(n_ref / 8 + 2, 0x99999999u);
	for (size_t i = 0; i < n_ref; ++i) S[i >> 3] = (S[i >> 3] & ~(0xfu << ((i & 7) << 2))) | ((uint32_t)(ref[i] & 0xf) << ((i & 7) << 2));
	return run_jobs(n_jobs, cig_off, n_cigar, cigars, long_min_cols, tile_cols, out, out_cap, res4,
	                [&](int j) { wmk::extra_src_pos P = { pk.data(), nm.data(), S.data(), (long long)qwin_off[j], (long long)t_base[j], q_pos[j], qwin_len[j] }; return P; });
}

} // extern "C"

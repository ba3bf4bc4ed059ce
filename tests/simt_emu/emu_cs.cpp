// tests/simt_emu/emu_cs.cpp — TEST INFRASTRUCTURE ONLY.
// The cs:Z / MD:Z bodies on the host wavefront emulator (winnowmap_amd/csrc/cs_kernel.h), launched the way csrc/wm_cs.hip launches them: prefix pass, the count pass in
// either class, the scan over jobs, the write pass. Byte form and position form. emu_cs_spec is the specification itself (cigar_cs.h).
#include <stdint.h>
#include "simt.h"                    // the emulator (this directory is first on the include path)
#include "cs_kernel.h"               // winnowmap_amd/csrc
#include "cigar_cs.h"
#include <vector>
#include <string.h>

#ifndef WM_EMU_CS_GUARD
#define WM_EMU_CS_GUARD 1            // bytes behind the output pool (0 in a sanitizer build: the pool and the sequence copy then have exactly the needed size)
#endif

namespace {
const int POISON = 0x5a5a5a5a;
struct Pre { std::vector<int> c, q, t, w; };

template <class MakeSrc>
long long run_jobs(int mode, int n_jobs, const uint32_t *cig_off, const int32_t *n_cigar, const uint32_t *cigars, int long_min_cols, int tile_cols, uint8_t *out, size_t out_cap,
                   int32_t *res4, const MakeSrc &make)
{
	std::vector<Pre> pre(n_jobs);
	std::vector<std::vector<int>> part(n_jobs);
	std::vector<int> cnt((size_t)n_jobs + 1, POISON);
	auto is_long = [&](int j) { return pre[j].c[n_cigar[j] + 1] >= long_min_cols; };
	for (int j = 0; j < n_jobs; ++j) {                                       // prefix + count
		const int n = n_cigar[j];
		const uint32_t *cig = cigars + cig_off[j];
		Pre &P = pre[j];
		P.c.assign(n + 2, POISON); P.q.assign(n + 1, POISON); P.t.assign(n + 1, POISON); P.w.assign(n + 1, POISON);      // a slot the kernels should not read shows
		simt::exec_mask() = ~0ull;
		wmk::cs_prefix(mode, cig, n, P.c.data(), P.q.data(), P.t.data(), P.w.data());
		const auto S = make(j);
		if (!is_long(j)) wmk::cs_short_count(S, mode, P.c.data(), P.q.data(), P.t.data(), P.w.data(), n, tile_cols, cnt.data() + j);
		else {
			const int n_tiles = (P.c[n + 1] + tile_cols - 1) / tile_cols;
			part[j].assign((size_t)n_tiles * 4, POISON);
			for (int tile = n_tiles - 1; tile >= 0; --tile)
				wmk::cs_long_count(S, mode, P.c.data(), P.q.data(), P.t.data(), P.w.data(), n, tile_cols, tile, part[j].data() + (size_t)tile * 4);
			wmk::cs_combine(part[j].data(), n_tiles, cnt.data() + j);
		}
	}
	int tot2[2] = { POISON, POISON };
	wmk::cs_job_scan(cnt.data(), n_jobs, res4, tot2);
	const long long total = (long long)(((unsigned long long)(unsigned)tot2[1] << 32) | (unsigned)tot2[0]);
	if ((size_t)total > out_cap) return total;
	std::vector<uint8_t> pool((size_t)total + WM_EMU_CS_GUARD, 0xee);         // exactly the reported size, a guard byte behind it
	for (int j = 0; j < n_jobs; ++j) {                                       // write
		const int n = n_cigar[j];
		Pre &P = pre[j];
		uint8_t *o = pool.data() + (((unsigned long long)(unsigned)res4[(size_t)j * 4 + 1] << 32) | (unsigned)res4[(size_t)j * 4]);
		const auto S = make(j);
		if (!is_long(j)) wmk::cs_short_write(S, mode, P.c.data(), P.q.data(), P.t.data(), P.w.data(), n, tile_cols, o);
		else
			for (int tile = (int)part[j].size() / 4 - 1; tile >= 0; --tile)
				wmk::cs_long_write(S, mode, P.c.data(), P.q.data(), P.t.data(), P.w.data(), n, tile_cols, tile, part[j].data() + (size_t)tile * 4, o);
	}
	if (WM_EMU_CS_GUARD && pool[total] != 0xee) return -1;                    // a store behind the call's output
	for (long long i = 0; i < total; ++i) if (pool[i] == 0xee) return -2;      // a byte nobody wrote (no tag holds this byte)
	if (total) memcpy(out, pool.data(), (size_t)total);
	return total;
}
} // namespace

extern "C" {

// the specification: the body of cig[0, n) at out (room for emu_cs_bound bytes); returns the bytes, or -(k + 1) for the op it refuses
long long emu_cs_spec(int mode, const uint32_t *cig, int n, const uint8_t *q, const uint8_t *t, char *out) { return wm_cigar_cs(mode, cig, n, q, t, out); }
long long emu_cs_bound(const uint32_t *cig, int n) { return wm_cigar_cs_bound(cig, n); }
int emu_cs_check(int mode, const uint32_t *cig, int n) { return wm_cigar_cs_check(mode, cig, n); }

// byte form: operands at seqs + q_off[j] / t_off[j]. Returns the bytes of the whole call (> out_cap: nothing written), res4 = wm_cs_res_t per job; < 0: see run_jobs
long long emu_cs_batch(int mode, int n_jobs, const uint32_t *q_off, const uint32_t *t_off, const uint32_t *cig_off, const int32_t *n_cigar, const uint8_t *seqs,
                       size_t seqs_bytes, const uint32_t *cigars, int long_min_cols, int tile_cols, uint8_t *out, size_t out_cap, int32_t *res4)
{
	std::vector<uint64_t> slab(WM_EMU_CS_GUARD ? seqs_bytes / 8 + 2 : (seqs_bytes + 7) / 8, 0x0909090909090909ULL);
	if (seqs_bytes) memcpy(slab.data(), seqs, seqs_bytes);
	const uint8_t *sq = (const uint8_t*)slab.data();
	return run_jobs(mode, n_jobs, cig_off, n_cigar, cigars, long_min_cols, tile_cols, out, out_cap, res4,
	                [&](int j) { wmk::extra_src_bytes S = { sq, (long long)q_off[j], (long long)t_off[j] }; return S; });
}

// position form: reads = 0..4 codes of the resident reads (packed here), ref = 0..15 codes of the reference, one per base (packed to nibbles here)
long long emu_cs_batch_pos(int mode, int n_jobs, const int64_t *qwin_off, const int32_t *qwin_len, const int32_t *q_pos, const int64_t *t_base, const uint32_t *cig_off,
                           const int32_t *n_cigar, const uint8_t *reads, size_t n_reads, const uint8_t *ref, size_t n_ref, const uint32_t *cigars, int long_min_cols,
                           int tile_cols, uint8_t *out, size_t out_cap, int32_t *res4)
{
	std::vector<uint64_t> pk(wm_pk_words(n_reads), 0), nm(wm_nm_words(n_reads), 0);
	wm_pack_codes(reads, n_reads, pk.data(), nm.data());
	std::vector<uint32_t> S(n_ref / 8 + 2, 0x99999999u);
	for (size_t i = 0; i < n_ref; ++i) S[i >> 3] = (S[i >> 3] & ~(0xfu << ((i & 7) << 2))) | ((uint32_t)(ref[i] & 0xf) << ((i & 7) << 2));
	return run_jobs(mode, n_jobs, cig_off, n_cigar, cigars, long_min_cols, tile_cols, out, out_cap, res4,
	                [&](int j) { wmk::extra_src_pos P = { pk.data(), nm.data(), S.data(), (long long)qwin_off[j], (long long)t_base[j], q_pos[j], qwin_len[j] }; return P; });
}

} // extern "C"

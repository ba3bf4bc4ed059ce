// tests/simt_emu/emu_sketchsteps.cpp — TEST INFRASTRUCTURE ONLY.
// The chunked sketch of a long sequence under homopolymer compression and / or at an even k (winnowmap_amd/csrc/sketch_kernel.h: sketch_steps_stage,
// sketch_steps_scan, then the two phases over slot space) on the host wavefront emulator: one emulated wavefront per chunk, stage after stage in the order
// of the launches of wm_index.hip's sketch_launch. Odd k without compression runs the plain chunked form (no stage at all), so one entry serves every mode.
#include <stdint.h>
#include "simt.h"                    // the emulator (this directory is first on the include path)
#include "sketch_kernel.h"           // winnowmap_amd/csrc
#include <algorithm>
#include <vector>

extern "C" {

// mm_sketch of n sequences (0..4 codes at seqs + offs[i]), each cut into chunks of `chunk` bases. packed != 0: the sequences live in a packed read buffer
// (reads2bit.h) behind a lead that is no multiple of 64 bases. Scratch of exactly len + 1 entries per array, poisoned. ranges (optional): per chunk
// (begin, end, sync) in slot space, sequence i's chunks from entry range_offs[i] on; sync = -1: the chunk was absorbed by the one before it (0 for a first chunk).
int emu_sketchsteps(int n, const uint8_t *seqs, const uint64_t *offs, const int32_t *lens, int w, int k, int hpc, int packed, uint32_t table_bits, uint32_t salt0, uint32_t salt1,
                    const uint8_t *bloom_bits, uint64_t *ox, uint64_t *oy, const uint64_t *out_offs, const int32_t *caps, int32_t *counts, int chunk, int32_t *ranges, const uint64_t *range_offs)
{
	uint64_t tot = 0;
	size_t bases = 0;
	for (int i = 0; i < n; ++i) { tot = std::max<uint64_t>(tot, out_offs[i] + caps[i]); if (lens[i] > 0) bases = std::max<size_t>(bases, (size_t)offs[i] + (size_t)lens[i]); }
	std::vector<wm128_t> out(tot + 1);
	const size_t lead = 37;
	std::vector<uint64_t> pk(1), nm(1);
	if (packed) {
		std::vector<uint8_t> buf(lead + bases + 5, 2);
		std::copy(seqs, seqs + bases, buf.begin() + lead);
		pk.assign(wm_pk_words(buf.size()), 0); nm.assign(wm_nm_words(buf.size()), 0);
		wm_pack_codes(buf.data(), buf.size(), pk.data(), nm.data());
	}
	wm_sketch_params_t P = { w, k, table_bits, salt0, salt1 };
	P.hpc = hpc;
	const bool even = !(k & 1), steps = hpc || even;
	const uint8_t *sq = packed ? 0 : seqs;
	for (int i = 0; i < n; ++i) {
		wm_sketch_job_t jb;
		jb.seq_off = packed ? (WM_RD_PACKED_BIT | (offs[i] + lead)) : offs[i]; jb.len = lens[i] > 0 ? lens[i] : 0; jb.out_off = out_offs[i]; jb.cap = caps[i]; jb.scratch_off = 0;
		const int len = jb.len, n_ch = len > 0 ? (len + chunk - 1) / chunk : 1;
		const size_t L = (size_t)len + 1;
		std::vector<double> so(L, -7.0); std::vector<uint64_t> sx(L, 0x1111); std::vector<uint32_t> sy(L, 0x2222), sl(L, 0x3333), he(L, 0xdeadbeefu), ei(L, 0xdeadbeefu);
		std::vector<uint8_t> hc(L, 9), nn(L, 9);
		std::vector<int> tab((size_t)6 * n_ch + 3, -12345), cb(n_ch), ce(n_ch), sync(n_ch, -1);
		wmk::wm_sk_steps_t T;
		for (int s = 0; s < 3; ++s) { T.cnt[s] = tab.data() + (size_t)s * n_ch; T.off[s] = tab.data() + (size_t)(3 + s) * n_ch; }
		T.tot = tab.data() + (size_t)6 * n_ch;
		for (int c = 0; c < n_ch; ++c) { cb[c] = c * chunk; ce[c] = std::min(len, (c + 1) * chunk); }
		simt::exec_mask() = ~0ull;
		auto stage = [&](int s, bool scatter) { for (int c = 0; c < n_ch; ++c) wmk::sketch_steps_stage(P, jb, sq, pk.data(), nm.data(), c, cb[c], ce[c], T, s, scatter, hc.data(), he.data(), nn.data(), ei.data()); };
		auto scan = [&](int s) { T.tot[s] = wmk::sketch_steps_scan(T.cnt[s], T.off[s], n_ch); };
		int slots = len;
		if (steps) {
			if (hpc) { stage(wmk::SK_RUNS, false); scan(wmk::SK_RUNS); stage(wmk::SK_RUNS, true); }
			if (even) {
				if (!hpc) stage(wmk::SK_CODES, false);
				scan(wmk::SK_CODES); stage(wmk::SK_CODES, true);
				stage(wmk::SK_SURV, false); scan(wmk::SK_SURV); stage(wmk::SK_SURV, true);
			}
			const int last = even ? wmk::SK_SURV : wmk::SK_RUNS;
			for (int c = 0; c < n_ch; ++c) { cb[c] = T.off[last][c]; ce[c] = cb[c] + T.cnt[last][c]; }      // (the chunk table in slot space)
			slots = T.tot[last];
		}
		for (int c = n_ch - 1; c >= 0; --c) {                     // (any order: phase 1 of a chunk depends on the steps alone)
			if (steps) wmk::sketch_p1_steps(P, (long long)jb.seq_off, slots, sq, pk.data(), nm.data(), bloom_bits, so.data(), sx.data(), sy.data(), sl.data(), cb[c], ce[c], hc.data(), he.data(), ei.data());
			else wmk::sketch_p1_range(P, (long long)jb.seq_off, slots, sq, pk.data(), nm.data(), bloom_bits, so.data(), sx.data(), sy.data(), sl.data(), cb[c], ce[c]);
		}
		sync[0] = 0;
		for (int c = 1; c < n_ch; ++c) sync[c] = wmk::sketch_find_sync(w, so.data(), cb[c], ce[c]);
		int total = 0;
		for (int c = 0; c < n_ch; ++c) {
			if (c > 0 && sync[c] < 0) continue;
			int t_stop = -1;
			for (int d = c + 1; d < n_ch && t_stop < 0; ++d) t_stop = sync[d];
			std::vector<wm128_t> tmp((size_t)len + 2);            // (a wavefront covers every chunk it absorbs)
			const int cnt = wmk::sketch_p2_range(P, slots, so.data(), sx.data(), sy.data(), sl.data(), c == 0 ? 0 : sync[c], c != 0, t_stop, tmp.data(), (int)tmp.size());
			if (cnt > (int)tmp.size()) return -1;
			for (int j = 0; j < cnt; ++j) { if (total < caps[i]) out[out_offs[i] + total] = tmp[j]; ++total; }
		}
		counts[i] = total;
		if (ranges) for (int c = 0; c < n_ch; ++c) { int32_t *r = ranges + 3 * (range_offs[i] + c); r[0] = cb[c]; r[1] = ce[c]; r[2] = sync[c]; }
	}
	for (uint64_t i = 0; i < tot; ++i) ox[i] = out[i].x, oy[i] = out[i].y;
	return 0;
}

} // extern "C"

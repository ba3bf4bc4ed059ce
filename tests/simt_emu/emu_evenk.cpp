// tests/simt_emu/emu_evenk.cpp — TEST INFRASTRUCTURE ONLY.
// The one-wavefront-per-sequence sketch (winnowmap_amd/csrc/sketch_kernel.h: sketch_coop) on the host wavefront emulator for an EVEN k: the steps that
// survive the palindrome rule of src/sketch.c:166 (sketch_even_steps), then the two phases over them; staged bytes and packed reads, with and without
// homopolymer compression. Event counters: steps skipped, and skips that fell while fewer than k steps had survived since the last ambiguous base.
#include <stdint.h>
static long long g_eev[2];
#define WM_EVENK_EVENT(skipped, low) (g_eev[0] += (skipped), g_eev[1] += (low))
#include "simt.h"                    // the emulator (this directory is first on the include path)
#include "sketch_kernel.h"           // winnowmap_amd/csrc
#include <algorithm>
#include <vector>

extern "C" {

void emu_evenk_events(long long *out) { out[0] = g_eev[0]; out[1] = g_eev[1]; }
void emu_evenk_events_clear(void) { g_eev[0] = g_eev[1] = 0; }

// mm_sketch of n sequences (0..4 codes at seqs + offs[i]) through sketch_coop; packed != 0: the sequences live in a packed read buffer (reads2bit.h) behind a
// lead that is no multiple of 64 bases. Scratch of exactly len + 1 entries per array, poisoned, so that a slot the kernel should not read shows.
int emu_evenk_sketch(int n, const uint8_t *seqs, const uint64_t *offs, const int32_t *lens, int w, int k, int hpc, int packed, uint32_t table_bits, uint32_t salt0, uint32_t salt1,
                     const uint8_t *bloom_bits, uint64_t *ox, uint64_t *oy, const uint64_t *out_offs, const int32_t *caps, int32_t *counts)
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
	for (int i = 0; i < n; ++i) {
		wm_sketch_job_t jb;
		jb.seq_off = packed ? (WM_RD_PACKED_BIT | (offs[i] + lead)) : offs[i]; jb.len = lens[i]; jb.out_off = out_offs[i]; jb.cap = caps[i]; jb.scratch_off = 0;
		const size_t L = (size_t)(lens[i] > 0 ? lens[i] : 0) + 1;
		std::vector<double> so(L, -7.0); std::vector<uint64_t> sx(L, 0x1111); std::vector<uint32_t> sy(L, 0x2222), sl(L, 0x3333), he(L, 0xdeadbeefu), ei(L, 0xdeadbeefu);
		std::vector<uint8_t> hc(L, 9), nn(L, 9);
		simt::exec_mask() = ~0ull;
		wmk::sketch_coop(P, jb, packed ? 0 : seqs, pk.data(), nm.data(), bloom_bits, so.data(), sx.data(), sy.data(), sl.data(), out.data(), counts + i, hc.data(), he.data(), nn.data(), ei.data());
	}
	for (uint64_t i = 0; i < tot; ++i) ox[i] = out[i].x, oy[i] = out[i].y;
	return 0;
}

} // extern "C"

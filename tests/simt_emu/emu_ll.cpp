// tests/simt_emu/emu_ll.cpp — TEST INFRASTRUCTURE ONLY.
// ksw_ll_i16 on the host wavefront emulator (winnowmap_amd/csrc/ll_kernel.h), routed the way csrc/wm_ll.hip routes it: a job whose padded query has at most reg_max
// positions runs in the register class, every other one in the LDS class. Byte form and position form. emu_ll_spec is the specification itself (ksw_ll.h).
#include <stdint.h>
#include "simt.h"                    // the emulator (this directory is first on the include path)
#include "ll_kernel.h"               // winnowmap_amd/csrc
#include "ksw_ll.h"
#include <vector>
#include <string.h>

namespace {
const int POISON = 0x5a5a5a5a;

template <class Src>
void run_job(const Src &S, int qlen, int tlen, const int8_t *mat, int gapo, int gape, int reg_max, int32_t *out3)
{
	int matw[25];
	for (int i = 0; i < 25; ++i) matw[i] = mat[i];
	const int n = (qlen + 7) / 8 * 8;
	simt::exec_mask() = ~0ull;
	if (n <= reg_max) wmk::ll_job<false>(S, qlen, tlen, matw, gapo + gape, gape, (int*)0, out3);
	else {
		std::vector<int> rows((size_t)2 * tlen, POISON);                   // exactly the job's rows: a slot the kernel should not read shows
		wmk::ll_job<true>(S, qlen, tlen, matw, gapo + gape, gape, rows.data(), out3);
	}
}
} // namespace

extern "C" {

int emu_ll_spec(int qlen, const uint8_t *q, int tlen, const uint8_t *t, const int8_t *mat, int gapo, int gape, int *qe, int *te)
{
	return wm_ksw_ll_spec(qlen, q, tlen, t, mat, gapo, gape, qe, te);
}

// byte form, the layout of wm_ll_job_t: job j's query is seqs[q_off[j], q_off[j] + qlen[j]), read from its first byte on (step 1) or from its last byte backwards
// (step -1), the target alike; out3 = {score, qe, te} per job. The slab is copied to its exact size.
void emu_ll_batch(int n_jobs, const int64_t *q_off, const int64_t *t_off, const int32_t *qlen, const int32_t *tlen, const int32_t *step, const uint8_t *seqs, size_t seqs_bytes,
                  const int8_t *mat, int gapo, int gape, int reg_max, int32_t *out3)
{
	std::vector<uint8_t> slab(seqs, seqs + seqs_bytes);
	for (int j = 0; j < n_jobs; ++j) {
		const wmk::ll_src_bytes S = { slab.data(), (long long)q_off[j] + (step[j] > 0 ? 0 : qlen[j] - 1), (long long)t_off[j] + (step[j] > 0 ? 0 : tlen[j] - 1), step[j] };
		run_job(S, qlen[j], tlen[j], mat, gapo, gape, reg_max, out3 + (size_t)3 * j);
	}
}

// position form: reads = 0..4 codes of the resident reads (packed here), ref = codes of the reference, one per base (packed to nibbles here)
void emu_ll_batch_pos(int n_jobs, const int64_t *qwin_off, const int32_t *qwin_len, const int32_t *q_pos, const int64_t *t_base, const int32_t *qlen, const int32_t *tlen,
                      const int32_t *step, const uint8_t *reads, size_t n_reads, const uint8_t *ref, size_t n_ref, const int8_t *mat, int gapo, int gape, int reg_max, int32_t *out3)
{
	std::vector<uint64_t> pk(wm_pk_words(n_reads), 0), nm(wm_nm_words(n_reads), 0);
	wm_pack_codes(reads, n_reads, pk.data(), nm.data());
	std::vector<uint32_t> S((n_ref + 7) / 8, 0x99999999u);
	for (size_t i = 0; i < n_ref; ++i) S[i >> 3] = (S[i >> 3] & ~(0xfu << ((i & 7) << 2))) | ((uint32_t)(ref[i] & 0xf) << ((i & 7) << 2));
	for (int j = 0; j < n_jobs; ++j) {
		const wmk::ll_src_pos P = { pk.data(), nm.data(), S.data(), (long long)qwin_off[j], (long long)t_base[j], q_pos[j], qwin_len[j], step[j] };
		run_job(P, qlen[j], tlen[j], mat, gapo, gape, reg_max, out3 + (size_t)3 * j);
	}
}

} // extern "C"

// final_src.h — where the entry points of the final-CIGAR kernels (wm_extra.hip, wm_eqx.hip, wm_cs.hip) find a job's operands: the call's byte slab, or the resident
// reads and the uploaded reference (extra_src_bytes / extra_src_pos of extra_kernel.h).
#pragma once
#include "simt.h"
#include "extra_kernel.h"

struct final_dev_src { const uint8_t *seqs; const uint64_t *pk, *nm; const uint32_t *S; };

// f(S) with job jb's operands in the form the call came in
template <bool POS, class F> WM_DEV void with_src(const final_dev_src &D, const wm_extra_djob_t &jb, F &&f)
{
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		f(S);
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		f(S);
	}
}

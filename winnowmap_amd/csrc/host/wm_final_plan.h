// wm_final_plan.h — the batch planner of the final-CIGAR device calls (wm_extra.hip, wm_eqx.hip, wm_cs.hip): validation of every job's CIGAR range and operands, the
// job records the kernels read, the prefix slots, and the split into the short and the long class. Host only — no HIP, no simt.h — so that the host harness
// (tests/host_harness/harness.cpp: wmh_final_plan_selftest) checks it without a device. What differs between the passes — how a job is measured, what it refuses on its
// own account — comes in as `measure`; where an error text goes comes in as `err` (the library's set_err, the harness's recorder).
#pragma once
#include <stdint.h>
#include <string.h>
#include <vector>
#include "../../../include/wm_gpu.h"

#define WM_EXTRA_GAP 64                     // bases of an I / D op per column (extra_kernel.h)

// one job as the kernels see it. Byte form: q_base / t_base = offsets of the operands in the call's sequence slab. Position form: q_base = first base of the (sub)read
// in the resident read codes, q_len its length, q_pos the two-strand index of the alignment's first query base; t_base = index of its first target base in the 4-bit S array
typedef struct { long long q_base, t_base; uint32_t cig_off, pre_off; int32_t n_cigar, q_pos, q_len, tile0; } wm_extra_djob_t;

// what the host needs to know of a job before it goes out (64-bit): columns, bases consumed, and the bound of the limit of extra_kernel.h
// (for mm_fix_cigar in front of the scan, fix_kernel.h: total = all lengths added up; bad_zero = the first op of length 0 and code >= 3, or -1)
typedef struct { int64_t cols, qlen, tlen, abs_sum, total; int32_t bad_zero; } wm_extra_measure_t;
static inline wm_extra_measure_t wm_extra_measure(const uint32_t *cig, int n, const wm_extra_score_t *sc)
{
	wm_extra_measure_t r = { 0, 0, 0, 0, 0, -1 };
	int64_t mx = sc->match < 0 ? -(int64_t)sc->match : sc->match, m_cols = 0;
	if (mx < (sc->mismatch < 0 ? -(int64_t)sc->mismatch : sc->mismatch)) mx = sc->mismatch < 0 ? -(int64_t)sc->mismatch : sc->mismatch;
	if (mx < (sc->ambi < 0 ? -(int64_t)sc->ambi : sc->ambi)) mx = sc->ambi < 0 ? -(int64_t)sc->ambi : sc->ambi;
	for (int k = 0; k < n; ++k) {
		const int64_t op = cig[k] & 0xf, len = cig[k] >> 4;
		r.total += len;
		if (len == 0 && op >= 3 && r.bad_zero < 0) r.bad_zero = k;
		if (op == 0) { m_cols += len; r.qlen += len; r.tlen += len; }
		else if (op == 1 || op == 2) {
			const int64_t g = (int64_t)sc->q + (int64_t)sc->e * len;
			r.cols += len > WM_EXTRA_GAP ? (len + WM_EXTRA_GAP - 1) / WM_EXTRA_GAP : 1;
			r.abs_sum += g < 0 ? -g : g;
			if (op == 1) r.qlen += len; else r.tlen += len;
		} else if (op == 3) r.tlen += len;
	}
	r.cols += m_cols; r.abs_sum += mx * m_cols;
	return r;
}

struct wm_final_pair { int32_t x, y; };     // tmap: { job, tile }; lmap: { job, its tiles } (an int2 on the device)
// what the position checks read from the context: the resident reads' extent and the contig table of the uploaded index
struct FinalView { size_t reads_bytes; const uint32_t *seq_len; const uint64_t *seq_off; size_t n_seq; };
// dj: one record per job; order: the short jobs; tmap / lmap: the long jobs' tiles (job i's from dj[i].tile0 on); n_pre: prefix entries, n_cigar + pre_slack per job, a
// slot of its own whatever the jobs' CIGAR ranges share
struct FinalPlan { std::vector<wm_extra_djob_t> dj; std::vector<int> order; std::vector<wm_final_pair> tmap, lmap; size_t n_pre; };
typedef int (*final_err_t)(int code, const char *fmt, ...);

// jobs (byte form) or pos (position form), one of them; measure(i, cig, nc, &qlen, &tlen, &cols) -> 0, or the code of its own refusal (through err). A job is long iff
// cols > 0 && cols >= long_min, in tiles of tile_cols columns. Returns WM_OK, or the code of the first refusal: the jobs behind it are not planned.
template <class Measure>
int final_plan(const FinalView &v, int n_jobs, const wm_extra_job_t *jobs, size_t seqs_bytes, const wm_extra_pos_t *pos, const uint32_t *cigars, size_t n_ops,
               int pre_slack, int long_min, int tile_cols, final_err_t err, Measure &&measure, FinalPlan &plan)
{
	plan.dj.assign((size_t)n_jobs, wm_extra_djob_t{});
	plan.order.clear(); plan.tmap.clear(); plan.lmap.clear();
	plan.n_pre = 0;
	for (int i = 0; i < n_jobs; ++i) {
		const uint32_t cig_off = pos ? pos[i].cig_off : jobs[i].cig_off;
		const int32_t nc = pos ? pos[i].n_cigar : jobs[i].n_cigar;
		if (nc < 0 || (uint64_t)cig_off + (uint64_t)nc > n_ops) return err(WM_EINVAL, "job %d: CIGAR ops [%u, %u + %d) outside the %zu ops of the call", i, cig_off, cig_off, nc, n_ops);
		int64_t qlen = 0, tlen = 0, cols = 0;
		if (const int rc = measure(i, cigars + cig_off, nc, &qlen, &tlen, &cols)) return rc;
		wm_extra_djob_t &d = plan.dj[i];
		d.cig_off = cig_off; d.n_cigar = nc; d.pre_off = (uint32_t)plan.n_pre;
		plan.n_pre += (size_t)nc + (size_t)pre_slack;
		if (plan.n_pre >= ((size_t)1 << 31)) return err(WM_ENOMEM, "batch holds 2^31 CIGAR ops or more; split it");
		if (pos) {
			const wm_extra_pos_t &s = pos[i];
			if (nc > 0) {
				if (s.qwin_off < 0 || s.qwin_len < 0 || s.qwin_len >= (1 << 30) || (uint64_t)s.qwin_off + (uint64_t)s.qwin_len > v.reads_bytes)
					return err(WM_EINVAL, "job %d: the (sub)read lies outside the resident reads", i);
				// (two-strand space is defined everywhere — outside [0, 2L) it reads N — but a CIGAR that leaves it by more than the few bases mm_align1_inv may step
				// in front of a strand is a caller's mistake; the target has no padding at all)
				if ((int64_t)s.q_pos < -16 || (int64_t)s.q_pos + qlen > 2 * (int64_t)s.qwin_len + 16)
					return err(WM_EINVAL, "job %d: the CIGAR consumes %lld query bases from two-strand position %d of a read of %d bases", i, (long long)qlen, s.q_pos, s.qwin_len);
				if (s.rid < 0 || (size_t)s.rid >= v.n_seq || s.t_pos < 0 || (int64_t)s.t_pos + tlen > (int64_t)v.seq_len[s.rid])
					return err(WM_EINVAL, "job %d: the CIGAR consumes %lld target bases from base %d of contig %d", i, (long long)tlen, s.t_pos, s.rid);
				d.q_base = s.qwin_off; d.q_pos = s.q_pos; d.q_len = s.qwin_len; d.t_base = (long long)v.seq_off[s.rid] + s.t_pos;
			}
		} else {
			const wm_extra_job_t &s = jobs[i];
			if (nc > 0 && ((uint64_t)s.q_off + (uint64_t)qlen > seqs_bytes || (uint64_t)s.t_off + (uint64_t)tlen > seqs_bytes))
				return err(WM_EINVAL, "job %d: the CIGAR consumes %lld query / %lld target bases, more than seqs holds behind its offsets", i, (long long)qlen, (long long)tlen);
			d.q_base = s.q_off; d.t_base = s.t_off;
		}
		if (cols > 0 && cols >= long_min) {
			const int64_t nt = (cols + tile_cols - 1) / tile_cols;
			if ((int64_t)plan.tmap.size() + nt >= ((int64_t)1 << 28)) return err(WM_ENOMEM, "batch holds more than 2^28 tiles; split it");      // (before the job's tiles go in)
			d.tile0 = (int32_t)plan.tmap.size();
			for (int32_t t = 0; t < (int32_t)nt; ++t) plan.tmap.push_back({ i, t });
			plan.lmap.push_back({ i, (int32_t)nt });
		} else plan.order.push_back(i);
	}
	return WM_OK;
}

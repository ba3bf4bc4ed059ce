// wm_extra.hip — libwmgpu.so, final-CIGAR unit: the scan of mm_update_extra (src/align.c:240-286) over batches of regions' final CIGARs — wm_extra_batch,
// wm_extra_batch_pos, wm_extra_set_routing of include/wm_gpu.h. The fold, the column space and the int32 argument are in extra_kernel.h; here are the kernel
// entry points, validation, the split into the two classes and the launches. (The mapper's switch and its counters live with the host mapper: host/wm_ops.cpp.)
// wm_fix_extra_batch / wm_fix_extra_batch_pos put mm_fix_cigar (src/align.c:91-167; fix_kernel.h, one wavefront per CIGAR) in front of the same scan: the stitched CIGARs
// go in, the fixed ones come out of a second pool, and the scan reads that pool with the operands advanced by both shifts.
#include "wm_rt.h"
#include "simt.h"
#include "extra_kernel.h"
#include "fix_kernel.h"

// ======================================================================================================
// kernels (one wavefront per workgroup)
// ======================================================================================================
struct extra_dev_src { const uint8_t *seqs; const uint64_t *pk, *nm; const uint32_t *S; };
struct extra_dev_pre { const uint32_t *cig; int *colS, *qS, *tS; };

// pass 1, every job: first column, qoff, toff of each op
__global__ __launch_bounds__(64) void extra_prefix_kernel(const wm_extra_djob_t *__restrict__ jobs, extra_dev_pre P)
{
	const wm_extra_djob_t jb = jobs[blockIdx.x];
	wmk::extra_prefix(P.cig + jb.cig_off, jb.n_cigar, P.colS + jb.pre_off, P.qS + jb.pre_off, P.tS + jb.pre_off);
}

// mm_fix_cigar, every job: raw CIGAR (P.cig, with pass 1's qS / tS) -> cig_out at the job's own cig_off, and { n_cigar, qshift, tshift, changed }; colS is its scratch
template <bool POS>
__global__ __launch_bounds__(64) void fix_kernel(const wm_extra_djob_t *__restrict__ jobs, extra_dev_src D, extra_dev_pre P, uint32_t *cig_out, wm_fix_res_t *res)
{
	const wm_extra_djob_t jb = jobs[blockIdx.x];
	const uint32_t *cig = P.cig + jb.cig_off;
	int *colS = P.colS + jb.pre_off;
	const int *qS = P.qS + jb.pre_off, *tS = P.tS + jb.pre_off;
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::fix_cigar_wave(S, cig, jb.n_cigar, qS, tS, colS, cig_out + jb.cig_off, (int*)(res + blockIdx.x));
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::fix_cigar_wave(S, cig, jb.n_cigar, qS, tS, colS, cig_out + jb.cig_off, (int*)(res + blockIdx.x));
	}
}
// ... then pass 1 again, over the fixed CIGAR: the job as the scan sees it (new count, operands advanced by both shifts; the query in two-strand space) -> jobs_out
template <bool POS>
__global__ __launch_bounds__(64) void fix_prefix_kernel(const wm_extra_djob_t *__restrict__ jobs, const wm_fix_res_t *__restrict__ res, wm_extra_djob_t *jobs_out, extra_dev_pre P)
{
	wm_extra_djob_t jb = jobs[blockIdx.x];
	const wm_fix_res_t fr = res[blockIdx.x];
	jb.n_cigar = fr.n_cigar; jb.t_base += fr.tshift;
	if (POS) jb.q_pos += fr.qshift; else jb.q_base += fr.qshift;
	if (threadIdx.x == 0) jobs_out[blockIdx.x] = jb;
	wmk::extra_prefix(P.cig + jb.cig_off, jb.n_cigar, P.colS + jb.pre_off, P.qS + jb.pre_off, P.tS + jb.pre_off);
}

// short class: workgroup g walks all tiles of job order[g]
template <bool POS>
__global__ __launch_bounds__(64) void extra_short_kernel(wm_extra_score_t sc, const wm_extra_djob_t *__restrict__ jobs, const int *__restrict__ order, extra_dev_src D,
                                                          extra_dev_pre P, int tile_cols, wm_extra_res_t *__restrict__ res)
{
	const int j = order[blockIdx.x];
	const wm_extra_djob_t jb = jobs[j];
	const uint32_t *cig = P.cig + jb.cig_off;
	const int *colS = P.colS + jb.pre_off, *qS = P.qS + jb.pre_off, *tS = P.tS + jb.pre_off;
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::extra_short(S, sc, cig, colS, qS, tS, jb.n_cigar, tile_cols, (int*)(res + j));
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::extra_short(S, sc, cig, colS, qS, tS, jb.n_cigar, tile_cols, (int*)(res + j));
	}
}

// long class: workgroup g folds tile tmap[g].y of job tmap[g].x into part[8 g ..]; then one workgroup per long job combines its tiles in order
template <bool POS>
__global__ __launch_bounds__(64) void extra_tile_kernel(wm_extra_score_t sc, const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ tmap, extra_dev_src D,
                                                         extra_dev_pre P, int tile_cols, int *__restrict__ part)
{
	const int2 tm = tmap[blockIdx.x];
	const wm_extra_djob_t jb = jobs[tm.x];
	const uint32_t *cig = P.cig + jb.cig_off;
	const int *colS = P.colS + jb.pre_off, *qS = P.qS + jb.pre_off, *tS = P.tS + jb.pre_off;
	int *out = part + (size_t)blockIdx.x * 8;
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::extra_long_tile(S, sc, cig, colS, qS, tS, jb.n_cigar, tile_cols, tm.y, out);
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::extra_long_tile(S, sc, cig, colS, qS, tS, jb.n_cigar, tile_cols, tm.y, out);
	}
}
__global__ __launch_bounds__(64) void extra_combine_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ lmap, extra_dev_pre P,
                                                            const int *__restrict__ part, wm_extra_res_t *__restrict__ res)
{
	const int2 lm = lmap[blockIdx.x];                          // { job, its tiles }
	const wm_extra_djob_t jb = jobs[lm.x];
	wmk::extra_combine(part + (size_t)jb.tile0 * 8, lm.y, P.qS + jb.pre_off, P.tS + jb.pre_off, jb.n_cigar, (int*)(res + lm.x));
}

// ======================================================================================================
// routing (process-wide; results never depend on it)
// ======================================================================================================
static std::atomic<int> g_extra_long_min(32768), g_extra_tile(512);
extern "C" void wm_extra_set_routing(int long_min_cols, int tile_cols)
{
	if (long_min_cols >= 0) g_extra_long_min = long_min_cols;
	if (tile_cols >= 64 && tile_cols % 64 == 0) g_extra_tile = tile_cols;
}
extern "C" int wm_extra_tile_cols(void) { return g_extra_tile.load(std::memory_order_relaxed); }
int extra_long_min_cols() { return g_extra_long_min.load(std::memory_order_relaxed); }      // (for wm_eqx.hip, which is routed by the same two values)

// ======================================================================================================
// the batched call
// ======================================================================================================
// fix_out != 0: mm_fix_cigar first (cigars = the stitched CIGARs, cigars_out = the fixed ones); then sc_in == 0 && out == 0 is the fix alone
static int extra_batch_impl(wm_ctx_t *c, const wm_extra_score_t *sc_in, int n_jobs, const wm_extra_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes,
                            const wm_extra_pos_t *pos, const uint32_t *cigars, size_t n_ops, wm_extra_res_t *out, uint32_t *cigars_out = 0, wm_fix_res_t *fix_out = 0)
try {
	const bool fix = fix_out != 0, scan = !fix || sc_in || out;
	if (!c) return set_err(WM_EINVAL, "null context");
	if (n_jobs < 0) return set_err(WM_EINVAL, "n_jobs < 0");
	if (n_jobs == 0) return WM_OK;
	if ((scan && (!sc_in || !out)) || (!jobs && !pos) || (n_ops && !cigars) || (jobs && seqs_bytes && !seqs) || (fix && n_ops && !cigars_out)) return set_err(WM_EINVAL, "null argument");
	if (pos && (!c->d_S || c->seq_len.empty())) return set_err(WM_EINVAL, "position jobs need wm_index_upload on this context");
	if (pos && !c->d_reads) return set_err(WM_EINVAL, "position jobs need wm_reads_upload on this context");
	if (n_ops >= ((size_t)1 << 31)) return set_err(WM_ENOMEM, "batch holds %zu CIGAR ops (limit 2^31 per batch)", n_ops);
	const wm_extra_score_t sc = scan ? *sc_in : wm_extra_score_t{ 0, 0, 0, 0, 0 };
	const int tile_cols = g_extra_tile.load(std::memory_order_relaxed), long_min = g_extra_long_min.load(std::memory_order_relaxed);
	HIPCHK(hipSetDevice(c->device));
	ArenaMark mark(c);
	const size_t nj = (size_t)n_jobs;
	std::vector<wm_extra_djob_t> dj(nj);
	std::vector<int> order; std::vector<int2> tmap, lmap;
	size_t n_pre = 0;                              // prefix entries: n_cigar + 1 per job, a slot of its own whatever the jobs' CIGAR ranges share
	for (int i = 0; i < n_jobs; ++i) {
		const uint32_t cig_off = pos ? pos[i].cig_off : jobs[i].cig_off;
		const int32_t nc = pos ? pos[i].n_cigar : jobs[i].n_cigar;
		if (nc < 0 || (uint64_t)cig_off + (uint64_t)nc > n_ops) return set_err(WM_EINVAL, "job %d: CIGAR ops [%u, %u + %d) outside the %zu ops of the call", i, cig_off, cig_off, nc, n_ops);
		// (a fused call is validated, sized and routed from the RAW CIGAR: mm_fix_cigar conserves the M columns and only merges or drops I / D ops, so neither the
		// bound below nor the column count grows; a long job's surplus tiles contribute the identity)
		const wm_extra_measure_t ms = wm_extra_measure(cigars + cig_off, nc, &sc);
		if (fix && ms.bad_zero >= 0)
			return set_err(WM_EINVAL, "job %d: op %d has length 0 and code %u (mm_fix_cigar indexes s[op] out of bounds there, src/align.c:132)", i, ms.bad_zero, cigars[cig_off + ms.bad_zero] & 0xf);
		if (fix && ms.total >= ((int64_t)1 << 31)) return set_err(WM_EINVAL, "job %d: the CIGAR's lengths add up to 2^31 or more", i);
		if (ms.abs_sum > WM_EXTRA_MAX_ABS)
			return set_err(WM_EINVAL, "job %d: max |score| x M columns + gap costs = %lld exceeds WM_EXTRA_MAX_ABS = 2^30 (the kernels' int32 arithmetic is exact below it)", i, (long long)ms.abs_sum);
		if (ms.cols >= ((int64_t)1 << 31) - 64 * (int64_t)tile_cols || ms.qlen >= ((int64_t)1 << 31) || ms.tlen >= ((int64_t)1 << 31))
			return set_err(WM_EINVAL, "job %d: the CIGAR spans 2^31 bases or more", i);
		wm_extra_djob_t &d = dj[i];
		memset(&d, 0, sizeof(d));
		d.cig_off = cig_off; d.n_cigar = nc; d.pre_off = (uint32_t)n_pre;
		n_pre += (size_t)nc + 1;
		if (n_pre >= ((size_t)1 << 31)) return set_err(WM_ENOMEM, "batch holds 2^31 CIGAR ops or more; split it");
		if (pos) {
			const wm_extra_pos_t &s = pos[i];
			if (nc > 0) {
				if (s.qwin_off < 0 || s.qwin_len < 0 || s.qwin_len >= (1 << 30) || (uint64_t)s.qwin_off + (uint64_t)s.qwin_len > c->reads_bytes)
					return set_err(WM_EINVAL, "job %d: the (sub)read lies outside the resident reads", i);
				// (two-strand space is defined everywhere — outside [0, 2L) it reads N — but a CIGAR that leaves it by more than the few bases mm_align1_inv may step
				// in front of a strand is a caller's mistake; the target has no padding at all)
				if ((int64_t)s.q_pos < -16 || (int64_t)s.q_pos + ms.qlen > 2 * (int64_t)s.qwin_len + 16)
					return set_err(WM_EINVAL, "job %d: the CIGAR consumes %lld query bases from two-strand position %d of a read of %d bases", i, (long long)ms.qlen, s.q_pos, s.qwin_len);
				if (s.rid < 0 || (size_t)s.rid >= c->seq_len.size() || s.t_pos < 0 || (int64_t)s.t_pos + ms.tlen > (int64_t)c->seq_len[s.rid])
					return set_err(WM_EINVAL, "job %d: the CIGAR consumes %lld target bases from base %d of contig %d", i, (long long)ms.tlen, s.t_pos, s.rid);
				d.q_base = s.qwin_off; d.q_pos = s.q_pos; d.q_len = s.qwin_len; d.t_base = (long long)c->seq_off[s.rid] + s.t_pos;
			}
		} else {
			const wm_extra_job_t &s = jobs[i];
			if (nc > 0 && ((uint64_t)s.q_off + (uint64_t)ms.qlen > seqs_bytes || (uint64_t)s.t_off + (uint64_t)ms.tlen > seqs_bytes))
				return set_err(WM_EINVAL, "job %d: the CIGAR consumes %lld query / %lld target bases, more than seqs holds behind its offsets", i, (long long)ms.qlen, (long long)ms.tlen);
			d.q_base = s.q_off; d.t_base = s.t_off;
		}
		if (ms.cols > 0 && ms.cols >= long_min) {
			const int nt = (int)((ms.cols + tile_cols - 1) / tile_cols);
			if (tmap.size() + (size_t)nt >= ((size_t)1 << 28)) return set_err(WM_ENOMEM, "batch holds more than 2^28 tiles; split it");
			d.tile0 = (int32_t)tmap.size();
			for (int t = 0; t < nt; ++t) tmap.push_back(make_int2(i, t));
			lmap.push_back(make_int2(i, nt));
		} else order.push_back(i);
	}
	const size_t n_short = order.size(), n_tiles = tmap.size(), n_long = lmap.size();
	wm_extra_djob_t *d_jobs = (wm_extra_djob_t*)arena_take(c, nj * sizeof(wm_extra_djob_t));
	wm_extra_res_t *d_res = (wm_extra_res_t*)arena_take(c, nj * sizeof(wm_extra_res_t));
	uint32_t *d_cig = (uint32_t*)arena_take(c, (n_ops + 16) * 4);
	uint32_t *d_cig2 = fix ? (uint32_t*)arena_take(c, (n_ops + 16) * 4) : 0;
	wm_extra_djob_t *d_jobs2 = fix ? (wm_extra_djob_t*)arena_take(c, nj * sizeof(wm_extra_djob_t)) : 0;
	wm_fix_res_t *d_fix = fix ? (wm_fix_res_t*)arena_take(c, nj * sizeof(wm_fix_res_t)) : 0;
	int *d_pre = (int*)arena_take(c, 3 * (n_pre + 16) * 4);
	int *d_order = (int*)arena_take(c, (n_short + 16) * 4);
	int2 *d_tmap = (int2*)arena_take(c, (n_tiles + n_long + 16) * sizeof(int2));
	int *d_part = (int*)arena_take(c, (n_tiles + 1) * 8 * 4);
	uint8_t *d_seqs = pos ? 0 : (uint8_t*)arena_take(c, seqs_bytes + 64);          // (+ slack: the word-wise gap scan reads to the end of the word that holds the last base)
	if (!d_jobs || !d_res || !d_cig || !d_pre || !d_order || !d_tmap || !d_part || (!pos && !d_seqs) || (fix && (!d_cig2 || !d_jobs2 || !d_fix)))
		return set_err(WM_ENOMEM, "extra batch (%zu ops, %zu tiles, %zu sequence bytes) does not fit the arena of %.1f MB; split it", n_ops, n_tiles, pos ? (size_t)0 : seqs_bytes, c->arena_bytes / 1048576.0);
	HIPCHK(hipMemcpyAsync(d_jobs, dj.data(), nj * sizeof(wm_extra_djob_t), hipMemcpyHostToDevice, c->stream));
	if (n_ops) HIPCHK(hipMemcpyAsync(d_cig, cigars, n_ops * 4, hipMemcpyHostToDevice, c->stream));
	if (n_short) HIPCHK(hipMemcpyAsync(d_order, order.data(), n_short * 4, hipMemcpyHostToDevice, c->stream));
	if (n_tiles) HIPCHK(hipMemcpyAsync(d_tmap, tmap.data(), n_tiles * sizeof(int2), hipMemcpyHostToDevice, c->stream));
	if (n_long) HIPCHK(hipMemcpyAsync(d_tmap + n_tiles, lmap.data(), n_long * sizeof(int2), hipMemcpyHostToDevice, c->stream));
	if (!pos && seqs_bytes) {
		HIPCHK(hipMemcpyAsync(d_seqs, seqs, seqs_bytes, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemsetAsync(d_seqs + seqs_bytes, 4, 64, c->stream));
	}
	extra_dev_pre P = { d_cig, d_pre, d_pre + (n_pre + 16), d_pre + 2 * (n_pre + 16) };
	const extra_dev_src D = { d_seqs, c->d_reads, c->d_reads_nm, c->d_S };
	hipLaunchKernelGGL(extra_prefix_kernel, dim3(n_jobs), dim3(64), 0, c->stream, d_jobs, P);
	if (fix) {
		if (pos) hipLaunchKernelGGL(fix_kernel<true>, dim3(n_jobs), dim3(64), 0, c->stream, d_jobs, D, P, d_cig2, d_fix);
		else hipLaunchKernelGGL(fix_kernel<false>, dim3(n_jobs), dim3(64), 0, c->stream, d_jobs, D, P, d_cig2, d_fix);
		HIPCHK(hipGetLastError());
		if (scan) {
			P.cig = d_cig2;
			if (pos) hipLaunchKernelGGL(fix_prefix_kernel<true>, dim3(n_jobs), dim3(64), 0, c->stream, d_jobs, d_fix, d_jobs2, P);
			else hipLaunchKernelGGL(fix_prefix_kernel<false>, dim3(n_jobs), dim3(64), 0, c->stream, d_jobs, d_fix, d_jobs2, P);
			d_jobs = d_jobs2;
		}
		if (n_ops) HIPCHK(hipMemcpyAsync(cigars_out, d_cig2, n_ops * 4, hipMemcpyDeviceToHost, c->stream));
		HIPCHK(hipMemcpyAsync(fix_out, d_fix, nj * sizeof(wm_fix_res_t), hipMemcpyDeviceToHost, c->stream));
	}
	if (scan && n_short) {
		if (pos) hipLaunchKernelGGL(extra_short_kernel<true>, dim3((unsigned)n_short), dim3(64), 0, c->stream, sc, d_jobs, d_order, D, P, tile_cols, d_res);
		else hipLaunchKernelGGL(extra_short_kernel<false>, dim3((unsigned)n_short), dim3(64), 0, c->stream, sc, d_jobs, d_order, D, P, tile_cols, d_res);
	}
	if (scan && n_tiles) {
		if (pos) hipLaunchKernelGGL(extra_tile_kernel<true>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, sc, d_jobs, d_tmap, D, P, tile_cols, d_part);
		else hipLaunchKernelGGL(extra_tile_kernel<false>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, sc, d_jobs, d_tmap, D, P, tile_cols, d_part);
		hipLaunchKernelGGL(extra_combine_kernel, dim3((unsigned)n_long), dim3(64), 0, c->stream, d_jobs, d_tmap + n_tiles, P, d_part, d_res);
	}
	HIPCHK(hipGetLastError());
	if (scan) HIPCHK(hipMemcpyAsync(out, d_res, nj * sizeof(wm_extra_res_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));
	return WM_OK;
}
catch (const std::bad_alloc &) { return set_err(WM_ENOMEM, "out of host memory"); }

// mm_update_extra's scan (src/align.c:240-286) over final CIGARs, operands as 0..4 codes inside seqs
extern "C" int wm_extra_batch(wm_ctx_t *c, const wm_extra_score_t *sc, int n_jobs, const wm_extra_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes,
                              const uint32_t *cigars, size_t n_ops, wm_extra_res_t *out)
{
	if (n_jobs > 0 && !jobs) return set_err(WM_EINVAL, "null jobs");
	return extra_batch_impl(c, sc, n_jobs, jobs, seqs, seqs_bytes, 0, cigars, n_ops, out);
}
// mm_update_extra's scan (src/align.c:240-286) over final CIGARs, operands as positions in the resident reads (two-strand space) and the uploaded reference
extern "C" int wm_extra_batch_pos(wm_ctx_t *c, const wm_extra_score_t *sc, int n_jobs, const wm_extra_pos_t *jobs, const uint32_t *cigars, size_t n_ops,
                                  wm_extra_res_t *out)
{
	if (n_jobs > 0 && !jobs) return set_err(WM_EINVAL, "null jobs");
	return extra_batch_impl(c, sc, n_jobs, 0, 0, 0, jobs, cigars, n_ops, out);
}

// mm_fix_cigar (src/align.c:91-167) and, unless score and extra_out are both NULL, mm_update_extra's scan (src/align.c:240-286) of the CIGAR it leaves; operands as 0..4 codes inside seqs
extern "C" int wm_fix_extra_batch(wm_ctx_t *c, const wm_extra_score_t *sc, int n_jobs, const wm_extra_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes,
                                  const uint32_t *cigars, size_t n_ops, uint32_t *cigars_out, wm_fix_res_t *fix_out, wm_extra_res_t *extra_out)
{
	if (n_jobs > 0 && (!jobs || !fix_out)) return set_err(WM_EINVAL, "null jobs or fix_out");
	if (n_jobs > 0 && !sc != !extra_out) return set_err(WM_EINVAL, "score and extra_out go together: both for the fused call, neither for the fix alone");
	return extra_batch_impl(c, sc, n_jobs, jobs, seqs, seqs_bytes, 0, cigars, n_ops, extra_out, cigars_out, fix_out);
}
// the same (src/align.c:91-167, :240-286), operands as positions in the resident reads (two-strand space) and the uploaded reference
extern "C" int wm_fix_extra_batch_pos(wm_ctx_t *c, const wm_extra_score_t *sc, int n_jobs, const wm_extra_pos_t *jobs, const uint32_t *cigars, size_t n_ops,
                                      uint32_t *cigars_out, wm_fix_res_t *fix_out, wm_extra_res_t *extra_out)
{
	if (n_jobs > 0 && (!jobs || !fix_out)) return set_err(WM_EINVAL, "null jobs or fix_out");
	if (n_jobs > 0 && !sc != !extra_out) return set_err(WM_EINVAL, "score and extra_out go together: both for the fused call, neither for the fix alone");
	return extra_batch_impl(c, sc, n_jobs, 0, 0, 0, jobs, cigars, n_ops, extra_out, cigars_out, fix_out);
}

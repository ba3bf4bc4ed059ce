// wm_cs.hip — libwmgpu.so, cs / MD unit: the bodies of the cs:Z / MD:Z tags (write_cs_core, write_MD_core, src/format.c:141-218, under --cs, --cs=long, --MD) over
// batches of regions' final CIGARs — wm_cs_batch, wm_cs_batch_pos of include/wm_gpu.h. The column space, the fold and the two passes are in cs_kernel.h, the
// specification in cigar_cs.h; here are the kernel entry points, what this pass measures and refuses of a job (what the reference asserts among it), and the launches;
// validation of ranges and operands and the split into the two classes by the values of wm_extra_set_routing are the planner's (host/wm_final_plan.h), the common uploads
// final_stage's (wm_rt.hip). (The mapper's switch and its counters live with the host mapper: host/wm_ops.cpp.)
#include "wm_rt.h"
#include "simt.h"
#include "cs_kernel.h"
#include "final_src.h"

// ======================================================================================================
// kernels (one wavefront per workgroup)
// ======================================================================================================
struct cs_dev_pre { const uint32_t *cig; int *cS, *qS, *tS, *wS; };

#define CS_JOB(j) \
	const wm_extra_djob_t jb = jobs[j]; \
	const int *cS = P.cS + jb.pre_off, *qS = P.qS + jb.pre_off, *tS = P.tS + jb.pre_off, *wS = P.wS + jb.pre_off

// pass 1, every job
__global__ __launch_bounds__(64) void cs_prefix_kernel(const wm_extra_djob_t *__restrict__ jobs, cs_dev_pre P, int mode)
{
	const wm_extra_djob_t jb = jobs[blockIdx.x];
	wmk::cs_prefix(mode, P.cig + jb.cig_off, jb.n_cigar, P.cS + jb.pre_off, P.qS + jb.pre_off, P.tS + jb.pre_off, P.wS + jb.pre_off);
}
// count, short class: workgroup g walks all tiles of job order[g] -> cnt[j]
template <bool POS>
__global__ __launch_bounds__(64) void cs_short_count_kernel(const wm_extra_djob_t *__restrict__ jobs, const int *__restrict__ order, final_dev_src D, cs_dev_pre P, int mode, int tile_cols, int *cnt)
{
	const int j = order[blockIdx.x];
	CS_JOB(j);
	with_src<POS>(D, jb, [&](const auto &S) { wmk::cs_short_count(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, cnt + j); });
}
// count, long class: workgroup g folds tile tmap[g].y of job tmap[g].x into part[4 g ..]; then one workgroup per long job turns its tiles' summaries into carries
template <bool POS>
__global__ __launch_bounds__(64) void cs_tile_count_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ tmap, final_dev_src D, cs_dev_pre P, int mode, int tile_cols, int *part)
{
	const int2 tm = tmap[blockIdx.x];
	CS_JOB(tm.x);
	int *out = part + (size_t)blockIdx.x * 4;
	with_src<POS>(D, jb, [&](const auto &S) { wmk::cs_long_count(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, tm.y, out); });
}
__global__ __launch_bounds__(64) void cs_combine_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ lmap, int *part, int *cnt)
{
	const int2 lm = lmap[blockIdx.x];                          // { job, its tiles }
	wmk::cs_combine(part + (size_t)jobs[lm.x].tile0 * 4, lm.y, cnt + lm.x);
}
// the scan over jobs (one workgroup)
__global__ __launch_bounds__(64) void cs_job_scan_kernel(const int *__restrict__ cnt, int n_jobs, wm_cs_res_t *res, int *total)
{
	static_assert(sizeof(wm_cs_res_t) == 16, "wm_cs_res_t is four ints for cs_job_scan");
	wmk::cs_job_scan(cnt, n_jobs, (int*)res, total);
}
// write
template <bool POS>
__global__ __launch_bounds__(64) void cs_short_write_kernel(const wm_extra_djob_t *__restrict__ jobs, const int *__restrict__ order, final_dev_src D, cs_dev_pre P, int mode, int tile_cols,
                                                             const wm_cs_res_t *__restrict__ res, uint8_t *out)
{
	const int j = order[blockIdx.x];
	CS_JOB(j);
	uint8_t *o = out + res[j].off;
	with_src<POS>(D, jb, [&](const auto &S) { wmk::cs_short_write(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, o); });
}
template <bool POS>
__global__ __launch_bounds__(64) void cs_tile_write_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ tmap, final_dev_src D, cs_dev_pre P, int mode, int tile_cols,
                                                            const int *__restrict__ part, const wm_cs_res_t *__restrict__ res, uint8_t *out)
{
	const int2 tm = tmap[blockIdx.x];
	CS_JOB(tm.x);
	uint8_t *o = out + res[tm.x].off;
	const int *pt = part + (size_t)blockIdx.x * 4;
	with_src<POS>(D, jb, [&](const auto &S) { wmk::cs_long_write(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, tm.y, pt, o); });
}

// ======================================================================================================
// the batched call
// ======================================================================================================
static int cs_batch_impl(wm_ctx_t *c, int mode, int n_jobs, const wm_extra_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes, const wm_extra_pos_t *pos, const uint32_t *cigars,
                         size_t n_ops, char *text_out, size_t out_cap, size_t *out_used, wm_cs_res_t *out)
try {
	if (!c) return set_err(WM_EINVAL, "null context");
	if (n_jobs < 0) return set_err(WM_EINVAL, "n_jobs < 0");
	if (mode != WM_CS_SHORT && mode != WM_CS_LONG && mode != WM_CS_MD) return set_err(WM_EINVAL, "mode %d is none of WM_CS_SHORT, WM_CS_LONG, WM_CS_MD", mode);
	if (out_used) *out_used = 0;
	if (n_jobs == 0) return WM_OK;
	if (!out || !out_used || (!jobs && !pos) || (n_ops && !cigars) || (jobs && seqs_bytes && !seqs) || (out_cap && !text_out)) return set_err(WM_EINVAL, "null argument");
	if (pos && (!c->d_S || c->seq_len.empty())) return set_err(WM_EINVAL, "position jobs need wm_index_upload on this context");
	if (pos && !c->d_reads) return set_err(WM_EINVAL, "position jobs need wm_reads_upload on this context");
	if (n_ops >= ((size_t)1 << 31)) return set_err(WM_ENOMEM, "batch holds %zu CIGAR ops (limit 2^31 per batch)", n_ops);
	const int tile_cols = wm_extra_tile_cols(), long_min = extra_long_min_cols();
	HIPCHK(hipSetDevice(c->device));
	ArenaMark mark(c);
	const size_t nj = (size_t)n_jobs;
	uint64_t bound_all = 0;
	auto measure = [&](int i, const uint32_t *cg, int nc, int64_t *qlen_out, int64_t *tlen_out, int64_t *cols_out) {
		const int bad = wm_cigar_cs_check(mode, cg, nc);
		if (bad >= 0) {
			if ((cg[bad] & 0xf) == 3) return set_err(WM_EINVAL, "job %d: op %d is an N of length %u, shorter than the 2 bases a cs tag prints on either side (src/format.c:180)", i, bad, cg[bad] >> 4);
			return set_err(WM_EINVAL, "job %d: op %d has code %u, outside M, I, D, N, =, X (src/format.c:147, :195)", i, bad, cg[bad] & 0xf);
		}
		int64_t qlen = 0, tlen = 0, cols = 1;                       // (the columns of cs_kernel.h: every printed gap base is one)
		for (int k = 0; k < nc; ++k) {
			const uint32_t op = cg[k] & 0xf;
			const int64_t len = cg[k] >> 4;
			if (op == 0 || op == 7 || op == 8) { qlen += len; tlen += len; cols += len + (mode == WM_CS_MD ? 0 : 1); }
			else if (op == 1) { qlen += len; cols += mode == WM_CS_MD ? 0 : len + 1; }
			else if (op == 2) { tlen += len; cols += len + 1; }
			else { tlen += len; cols += mode == WM_CS_MD ? 0 : 1; }
		}
		const int64_t bound = wm_cigar_cs_bound(cg, nc);
		if (bound >= ((int64_t)1 << 31) || cols >= ((int64_t)1 << 31) - 64 * (int64_t)tile_cols || qlen >= ((int64_t)1 << 31) || tlen >= ((int64_t)1 << 31))
			return set_err(WM_EINVAL, "job %d: the tag of this CIGAR can reach %lld bytes, 2^31 or more", i, (long long)bound);
		bound_all += (uint64_t)bound;
		*qlen_out = qlen; *tlen_out = tlen; *cols_out = cols;
		return 0;
	};
	FinalPlan plan;
	if (const int rc = final_plan(final_view(c), n_jobs, jobs, seqs_bytes, pos, cigars, n_ops, 2, long_min, tile_cols, set_err, measure, plan)) return rc;
	const size_t n_short = plan.order.size(), n_tiles = plan.tmap.size(), n_long = plan.lmap.size();
	wm_cs_res_t *d_res = (wm_cs_res_t*)arena_take(c, nj * sizeof(wm_cs_res_t));
	int *d_cnt = (int*)arena_take(c, (nj + 16) * 4);
	int *d_total = (int*)arena_take(c, 64);
	int *d_part = (int*)arena_take(c, (n_tiles + 1) * 4 * 4);
	FinalDev V;
	const int staged = d_res && d_cnt && d_total && d_part ? final_stage(c, plan, cigars, n_ops, seqs, seqs_bytes, pos, 4, &V) : WM_ENOMEM;
	if (staged == WM_ENOMEM)
		return set_err(WM_ENOMEM, "cs batch (%zu ops, %zu tiles, %zu sequence bytes) does not fit the arena of %.1f MB; split it", n_ops, n_tiles, pos ? (size_t)0 : seqs_bytes, c->arena_bytes / 1048576.0);
	if (staged) return staged;
	const wm_extra_djob_t *d_jobs = V.jobs;
	const size_t ps = V.pre_stride;
	const cs_dev_pre P = { V.cig, V.pre, V.pre + ps, V.pre + 2 * ps, V.pre + 3 * ps };
	const final_dev_src D = { V.seqs, c->d_reads, c->d_reads_nm, c->d_S };
	// ---- count ----
	hipLaunchKernelGGL(cs_prefix_kernel, dim3(n_jobs), dim3(64), 0, c->stream, d_jobs, P, mode);
	if (n_short) {
		if (pos) hipLaunchKernelGGL(cs_short_count_kernel<true>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, V.order, D, P, mode, tile_cols, d_cnt);
		else hipLaunchKernelGGL(cs_short_count_kernel<false>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, V.order, D, P, mode, tile_cols, d_cnt);
	}
	if (n_tiles) {
		if (pos) hipLaunchKernelGGL(cs_tile_count_kernel<true>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, V.tmap, D, P, mode, tile_cols, d_part);
		else hipLaunchKernelGGL(cs_tile_count_kernel<false>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, V.tmap, D, P, mode, tile_cols, d_part);
		hipLaunchKernelGGL(cs_combine_kernel, dim3((unsigned)n_long), dim3(64), 0, c->stream, d_jobs, V.lmap, d_part, d_cnt);
	}
	hipLaunchKernelGGL(cs_job_scan_kernel, dim3(1), dim3(64), 0, c->stream, d_cnt, n_jobs, d_res, d_total);
	HIPCHK(hipGetLastError());
	std::vector<wm_cs_res_t> res(nj);                                  // (out[] stays untouched when the arena refuses the write pass: a refused batch is split and issued again)
	HIPCHK(hipMemcpyAsync(res.data(), d_res, nj * sizeof(wm_cs_res_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));
	const uint64_t total = res[nj - 1].off + (uint64_t)res[nj - 1].len;
	*out_used = (size_t)total;
	if (total > bound_all) return set_err(WM_ENODEV, "internal: the count pass reports %llu bytes, more than the %llu the batch can have", (unsigned long long)total, (unsigned long long)bound_all);
	if (total > out_cap) { memcpy(out, res.data(), nj * sizeof(wm_cs_res_t)); return set_err(WM_ENOMEM, "text_out holds %zu bytes, the batch needs %llu", out_cap, (unsigned long long)total); }
	if (total == 0) { memcpy(out, res.data(), nj * sizeof(wm_cs_res_t)); return WM_OK; }
	// ---- write: every job walks its columns again, every lane from its own byte offset ----
	uint8_t *d_out = (uint8_t*)arena_take(c, (size_t)total + 64);
	if (!d_out) return set_err(WM_ENOMEM, "cs batch (%llu bytes out) does not fit the arena of %.1f MB; split it", (unsigned long long)total, c->arena_bytes / 1048576.0);
	memcpy(out, res.data(), nj * sizeof(wm_cs_res_t));
	if (n_short) {
		if (pos) hipLaunchKernelGGL(cs_short_write_kernel<true>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, V.order, D, P, mode, tile_cols, d_res, d_out);
		else hipLaunchKernelGGL(cs_short_write_kernel<false>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, V.order, D, P, mode, tile_cols, d_res, d_out);
	}
	if (n_tiles) {
		if (pos) hipLaunchKernelGGL(cs_tile_write_kernel<true>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, V.tmap, D, P, mode, tile_cols, d_part, d_res, d_out);
		else hipLaunchKernelGGL(cs_tile_write_kernel<false>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, V.tmap, D, P, mode, tile_cols, d_part, d_res, d_out);
	}
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(text_out, d_out, (size_t)total, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));
	return WM_OK;
}
catch (const std::bad_alloc &) { return set_err(WM_ENOMEM, "out of host memory"); }

// write_cs_core / write_MD_core (src/format.c:141-218) over final CIGARs, operands as 0..4 codes inside seqs
extern "C" int wm_cs_batch(wm_ctx_t *c, int mode, int n_jobs, const wm_extra_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes, const uint32_t *cigars, size_t n_ops,
                           char *text_out, size_t out_cap, size_t *out_used, wm_cs_res_t *out)
{
	if (n_jobs > 0 && !jobs) return set_err(WM_EINVAL, "null jobs");
	return cs_batch_impl(c, mode, n_jobs, jobs, seqs, seqs_bytes, 0, cigars, n_ops, text_out, out_cap, out_used, out);
}
// write_cs_core / write_MD_core (src/format.c:141-218) over final CIGARs, operands as positions in the resident reads (two-strand space) and the uploaded reference
extern "C" int wm_cs_batch_pos(wm_ctx_t *c, int mode, int n_jobs, const wm_extra_pos_t *jobs, const uint32_t *cigars, size_t n_ops,
                               char *text_out, size_t out_cap, size_t *out_used, wm_cs_res_t *out)
{
	if (n_jobs > 0 && !jobs) return set_err(WM_EINVAL, "null jobs");
	return cs_batch_impl(c, mode, n_jobs, 0, 0, 0, jobs, cigars, n_ops, text_out, out_cap, out_used, out);
}

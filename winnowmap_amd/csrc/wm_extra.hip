// wm_extra.hip — libwmgpu.so, final-CIGAR unit: the scan of mm_update_extra (src/align.c:240-286) over batches of regions' final CIGARs — wm_extra_batch,
// wm_extra_batch_pos, wm_extra_set_routing of include/wm_gpu.h. The fold, the column space and the int32 argument are in extra_kernel.h; here are the kernel
// entry points, what this pass measures and refuses of a job, and the launches; validation of ranges and operands and the split into the two classes are the
// planner's (host/wm_final_plan.h), the common uploads final_stage's (wm_rt.hip). (The mapper's switch and its counters live with the host mapper: host/wm_ops.cpp.)
// wm_fix_extra_batch / wm_fix_extra_batch_pos put mm_fix_cigar (src/align.c:91-167; fix_kernel.h, one wavefront per CIGAR) in front of the same scan: the stitched CIGARs
// go in, the fixed ones come out of a second pool, and the scan reads that pool with the operands advanced by both shifts.
#include "wm_rt.h"
#include "simt.h"
#include "extra_kernel.h"
#include "final_src.h"
#include "fix_kernel.h"

// ======================================================================================================
// kernels (one wavefront per workgroup)
// ======================================================================================================
struct extra_dev_pre { const uint32_t *cig; int *colS, *qS, *tS; };

// pass 1, every job: first column, qoff, toff of each op
__global__ __launch_bounds__(64) void extra_prefix_kernel(const wm_extra_djob_t *__restrict__ jobs, extra_dev_pre P)
{
	const wm_extra_djob_t jb = jobs[blockIdx.x];
	wmk::extra_prefix(P.cig + jb.cig_off, jb.n_cigar, P.colS + jb.pre_off, P.qS + jb.pre_off, P.tS + jb.pre_off);
}

// mm_fix_cigar, every job: raw CIGAR (P.cig, with pass 1's qS / tS) -> cig_out at the job's own cig_off, and { n_cigar, qshift, tshift, changed }; colS is its scratch
template <bool POS>
__global__ __launch_bounds__(64) void fix_kernel(const wm_extra_djob_t *__restrict__ jobs, final_dev_src D, extra_dev_pre P, uint32_t *cig_out, wm_fix_res_t *res)
{
	const wm_extra_djob_t jb = jobs[blockIdx.x];
	const uint32_t *cig = P.cig + jb.cig_off;
	int *colS = P.colS + jb.pre_off;
	const int *qS = P.qS + jb.pre_off, *tS = P.tS + jb.pre_off;
	with_src<POS>(D, jb, [&](const auto &S) { wmk::fix_cigar_wave(S, cig, jb.n_cigar, qS, tS, colS, cig_out + jb.cig_off, (int*)(res + blockIdx.x)); });
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
__global__ __launch_bounds__(64) void extra_short_kernel(wm_extra_score_t sc, const wm_extra_djob_t *__restrict__ jobs, const int *__restrict__ order, final_dev_src D,
                                                          extra_dev_pre P, int tile_cols, wm_extra_res_t *__restrict__ res)
{
	const int j = order[blockIdx.x];
	const wm_extra_djob_t jb = jobs[j];
	const uint32_t *cig = P.cig + jb.cig_off;
	const int *colS = P.colS + jb.pre_off, *qS = P.qS + jb.pre_off, *tS = P.tS + jb.pre_off;
	with_src<POS>(D, jb, [&](const auto &S) { wmk::extra_short(S, sc, cig, colS, qS, tS, jb.n_cigar, tile_cols, (int*)(res + j)); });
}

// long class: workgroup g folds tile tmap[g].y of job tmap[g].x into part[8 g ..]; then one workgroup per long job combines its tiles in order
template <bool POS>
__global__ __launch_bounds__(64) void extra_tile_kernel(wm_extra_score_t sc, const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ tmap, final_dev_src D,
                                                         extra_dev_pre P, int tile_cols, int *__restrict__ part)
{
	const int2 tm = tmap[blockIdx.x];
	const wm_extra_djob_t jb = jobs[tm.x];
	const uint32_t *cig = P.cig + jb.cig_off;
	const int *colS = P.colS + jb.pre_off, *qS = P.qS + jb.pre_off, *tS = P.tS + jb.pre_off;
	int *out = part + (size_t)blockIdx.x * 8;
	with_src<POS>(D, jb, [&](const auto &S) { wmk::extra_long_tile(S, sc, cig, colS, qS, tS, jb.n_cigar, tile_cols, tm.y, out); });
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
int extra_long_min_cols() { return g_extra_long_min.load(std::memory_order_relaxed); }      // (wm_eqx.hip and wm_cs.hip are routed by the same two values)

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
	// (a fused call is validated, sized and routed from the RAW CIGAR: mm_fix_cigar conserves the M columns and only merges or drops I / D ops, so neither the
	// bound below nor the column count grows; a long job's surplus tiles contribute the identity)
	auto measure = [&](int i, const uint32_t *cig, int nc, int64_t *qlen, int64_t *tlen, int64_t *cols) {
		const wm_extra_measure_t ms = wm_extra_measure(cig, nc, &sc);
		if (fix && ms.bad_zero >= 0)
			return set_err(WM_EINVAL, "job %d: op %d has length 0 and code %u (mm_fix_cigar indexes s[op] out of bounds there, src/align.c:132)", i, ms.bad_zero, cig[ms.bad_zero] & 0xf);
		if (fix && ms.total >= ((int64_t)1 << 31)) return set_err(WM_EINVAL, "job %d: the CIGAR's lengths add up to 2^31 or more", i);
		if (ms.abs_sum > WM_EXTRA_MAX_ABS)
			return set_err(WM_EINVAL, "job %d: max |score| x M columns + gap costs = %lld exceeds WM_EXTRA_MAX_ABS = 2^30 (the kernels' int32 arithmetic is exact below it)", i, (long long)ms.abs_sum);
		if (ms.cols >= ((int64_t)1 << 31) - 64 * (int64_t)tile_cols || ms.qlen >= ((int64_t)1 << 31) || ms.tlen >= ((int64_t)1 << 31))
			return set_err(WM_EINVAL, "job %d: the CIGAR spans 2^31 bases or more", i);
		*qlen = ms.qlen; *tlen = ms.tlen; *cols = ms.cols;
		return 0;
	};
	FinalPlan plan;
	if (const int rc = final_plan(final_view(c), n_jobs, jobs, seqs_bytes, pos, cigars, n_ops, 1, long_min, tile_cols, set_err, measure, plan)) return rc;
	const size_t n_short = plan.order.size(), n_tiles = plan.tmap.size(), n_long = plan.lmap.size();
	wm_extra_res_t *d_res = (wm_extra_res_t*)arena_take(c, nj * sizeof(wm_extra_res_t));
	uint32_t *d_cig2 = fix ? (uint32_t*)arena_take(c, (n_ops + 16) * 4) : 0;
	wm_extra_djob_t *d_jobs2 = fix ? (wm_extra_djob_t*)arena_take(c, nj * sizeof(wm_extra_djob_t)) : 0;
	wm_fix_res_t *d_fix = fix ? (wm_fix_res_t*)arena_take(c, nj * sizeof(wm_fix_res_t)) : 0;
	int *d_part = (int*)arena_take(c, (n_tiles + 1) * 8 * 4);
	FinalDev V;
	const int staged = d_res && d_part && (!fix || (d_cig2 && d_jobs2 && d_fix)) ? final_stage(c, plan, cigars, n_ops, seqs, seqs_bytes, pos, 3, &V) : WM_ENOMEM;
	if (staged == WM_ENOMEM)
		return set_err(WM_ENOMEM, "extra batch (%zu ops, %zu tiles, %zu sequence bytes) does not fit the arena of %.1f MB; split it", n_ops, n_tiles, pos ? (size_t)0 : seqs_bytes, c->arena_bytes / 1048576.0);
	if (staged) return staged;
	const wm_extra_djob_t *d_jobs = V.jobs;
	extra_dev_pre P = { V.cig, V.pre, V.pre + V.pre_stride, V.pre + 2 * V.pre_stride };
	const final_dev_src D = { V.seqs, c->d_reads, c->d_reads_nm, c->d_S };
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
		if (pos) hipLaunchKernelGGL(extra_short_kernel<true>, dim3((unsigned)n_short), dim3(64), 0, c->stream, sc, d_jobs, V.order, D, P, tile_cols, d_res);
		else hipLaunchKernelGGL(extra_short_kernel<false>, dim3((unsigned)n_short), dim3(64), 0, c->stream, sc, d_jobs, V.order, D, P, tile_cols, d_res);
	}
	if (scan && n_tiles) {
		if (pos) hipLaunchKernelGGL(extra_tile_kernel<true>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, sc, d_jobs, V.tmap, D, P, tile_cols, d_part);
		else hipLaunchKernelGGL(extra_tile_kernel<false>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, sc, d_jobs, V.tmap, D, P, tile_cols, d_part);
		hipLaunchKernelGGL(extra_combine_kernel, dim3((unsigned)n_long), dim3(64), 0, c->stream, d_jobs, V.lmap, P, d_part, d_res);
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

// wm_eqx.hip — libwmgpu.so, = / X unit: mm_update_cigar_eqx (src/align.c:169-238, the tail of mm_update_extra under MM_F_EQX, :285) over batches of regions' final
// CIGARs — wm_eqx_batch, wm_eqx_batch_pos of include/wm_gpu.h. The fold, the two passes and the slot arithmetic are in eqx_kernel.h, the specification in cigar_eqx.h;
// here are the kernel entry points, what this pass measures and refuses of a job, and the launches; validation of ranges and operands and the split into the two classes by
// the values of wm_extra_set_routing are the planner's (host/wm_final_plan.h), the common uploads final_stage's (wm_rt.hip).
// (The mapper's switch and its counters live with the host mapper: host/wm_ops.cpp.)
#include "wm_rt.h"
#include "simt.h"
#include "eqx_kernel.h"
#include "final_src.h"

// ======================================================================================================
// kernels (one wavefront per workgroup)
// ======================================================================================================
struct eqx_dev_pre { const uint32_t *cig; int *mS, *qS, *tS, *cS, *gS; };

#define EQX_JOB(j) \
	const wm_extra_djob_t jb = jobs[j]; \
	const uint32_t *cig = P.cig + jb.cig_off; \
	const int *mS = P.mS + jb.pre_off, *qS = P.qS + jb.pre_off, *tS = P.tS + jb.pre_off, *cS = P.cS + jb.pre_off; \
	int *gS = P.gS + jb.pre_off; (void)gS; (void)mS; (void)qS; (void)tS; (void)cig

// pass 1, every job
__global__ __launch_bounds__(64) void eqx_prefix_kernel(const wm_extra_djob_t *__restrict__ jobs, eqx_dev_pre P)
{
	const wm_extra_djob_t jb = jobs[blockIdx.x];
	wmk::eqx_prefix(P.cig + jb.cig_off, jb.n_cigar, P.mS + jb.pre_off, P.qS + jb.pre_off, P.tS + jb.pre_off, P.cS + jb.pre_off, P.gS + jb.pre_off);
}
// count, short class: workgroup g walks all tiles of job order[g] -> cnt[3 j ..]
template <bool POS>
__global__ __launch_bounds__(64) void eqx_short_count_kernel(const wm_extra_djob_t *__restrict__ jobs, const int *__restrict__ order, final_dev_src D, eqx_dev_pre P, int tile_cols, int *cnt)
{
	const int j = order[blockIdx.x];
	EQX_JOB(j);
	with_src<POS>(D, jb, [&](const auto &S) { wmk::eqx_short_count(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, cnt + (size_t)j * 3); });
}
// count, long class: workgroup g folds tile tmap[g].y of job tmap[g].x into part[2 g ..]; then one workgroup per long job turns its tiles' tuples into carries
template <bool POS>
__global__ __launch_bounds__(64) void eqx_tile_count_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ tmap, final_dev_src D, eqx_dev_pre P, int tile_cols, int *part)
{
	const int2 tm = tmap[blockIdx.x];
	EQX_JOB(tm.x);
	int *out = part + (size_t)blockIdx.x * 2;
	with_src<POS>(D, jb, [&](const auto &S) { wmk::eqx_long_count(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, tm.y, out); });
}
__global__ __launch_bounds__(64) void eqx_combine_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ lmap, eqx_dev_pre P, int *part, int *cnt)
{
	const int2 lm = lmap[blockIdx.x];                          // { job, its tiles }
	EQX_JOB(lm.x);
	wmk::eqx_combine(part + (size_t)jb.tile0 * 2, lm.y, cS, jb.n_cigar, cnt + (size_t)lm.x * 3);
}
// the scan over jobs (one workgroup)
__global__ __launch_bounds__(64) void eqx_job_scan_kernel(const int *__restrict__ cnt, int n_jobs, wm_eqx_res_t *res, int *total)
{
	static_assert(sizeof(wm_eqx_res_t) == 16, "wm_eqx_res_t is four ints for eqx_job_scan");
	wmk::eqx_job_scan(cnt, n_jobs, (int*)res, total);
}
// write, the jobs of the rewrite branch: the runs, and gS
template <bool POS>
__global__ __launch_bounds__(64) void eqx_short_write_kernel(const wm_extra_djob_t *__restrict__ jobs, const int *__restrict__ order, final_dev_src D, eqx_dev_pre P, int tile_cols,
                                                              const wm_eqx_res_t *__restrict__ res, uint32_t *out)
{
	const int j = order[blockIdx.x];
	EQX_JOB(j);
	uint32_t *o = out + res[j].off;
	with_src<POS>(D, jb, [&](const auto &S) { wmk::eqx_short_write(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, o, gS); });
}
template <bool POS>
__global__ __launch_bounds__(64) void eqx_tile_write_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ tmap, final_dev_src D, eqx_dev_pre P, int tile_cols,
                                                             const int *__restrict__ part, const wm_eqx_res_t *__restrict__ res, uint32_t *out)
{
	const int2 tm = tmap[blockIdx.x];                          // (the tiles of the rewrite-branch jobs only: { job, tile })
	EQX_JOB(tm.x);
	uint32_t *o = out + res[tm.x].off;
	const int *pt = part + ((size_t)jb.tile0 + (size_t)tm.y) * 2;
	with_src<POS>(D, jb, [&](const auto &S) { wmk::eqx_long_write(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, tm.y, pt, o, gS); });
}
// every job: the in-place relabelling, or the ops of another code between the runs
__global__ __launch_bounds__(64) void eqx_ops_kernel(const wm_extra_djob_t *__restrict__ jobs, eqx_dev_pre P, const wm_eqx_res_t *__restrict__ res, uint32_t *out)
{
	EQX_JOB(blockIdx.x);
	const wm_eqx_res_t r = res[blockIdx.x];
	wmk::eqx_ops_write(cig, jb.n_cigar, cS, gS, r.in_place, out + r.off);
}

// ======================================================================================================
// the batched call
// ======================================================================================================
static int eqx_batch_impl(wm_ctx_t *c, int n_jobs, const wm_extra_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes, const wm_extra_pos_t *pos, const uint32_t *cigars,
                          size_t n_ops, uint32_t *cigars_out, size_t out_cap, size_t *out_used, wm_eqx_res_t *out)
try {
	if (!c) return set_err(WM_EINVAL, "null context");
	if (n_jobs < 0) return set_err(WM_EINVAL, "n_jobs < 0");
	if (out_used) *out_used = 0;
	if (n_jobs == 0) return WM_OK;
	if (!out || !out_used || (!jobs && !pos) || (n_ops && !cigars) || (jobs && seqs_bytes && !seqs) || (out_cap && !cigars_out)) return set_err(WM_EINVAL, "null argument");
	if (pos && (!c->d_S || c->seq_len.empty())) return set_err(WM_EINVAL, "position jobs need wm_index_upload on this context");
	if (pos && !c->d_reads) return set_err(WM_EINVAL, "position jobs need wm_reads_upload on this context");
	if (n_ops >= ((size_t)1 << 31)) return set_err(WM_ENOMEM, "batch holds %zu CIGAR ops (limit 2^31 per batch)", n_ops);
	const int tile_cols = wm_extra_tile_cols(), long_min = extra_long_min_cols();
	const wm_extra_score_t sc0 = { 0, 0, 0, 0, 0 };
	HIPCHK(hipSetDevice(c->device));
	ArenaMark mark(c);
	const size_t nj = (size_t)n_jobs;
	std::vector<int64_t> mcols(nj);
	uint64_t bound = 0;                            // ops the call can write at most: every op, and one more per M column
	auto measure = [&](int i, const uint32_t *cig, int nc, int64_t *qlen, int64_t *tlen, int64_t *cols) {
		const wm_extra_measure_t ms = wm_extra_measure(cig, nc, &sc0);
		int64_t m = 0;
		for (int k = 0; k < nc; ++k) if ((cig[k] & 0xf) == 0) m += cig[k] >> 4;
		if (m >= ((int64_t)1 << 31) - 64 * (int64_t)tile_cols || ms.qlen >= ((int64_t)1 << 31) || ms.tlen >= ((int64_t)1 << 31))
			return set_err(WM_EINVAL, "job %d: the CIGAR spans 2^31 bases or more", i);
		mcols[i] = m;
		bound += (uint64_t)nc + (uint64_t)m;
		*qlen = ms.qlen; *tlen = ms.tlen; *cols = m;
		return 0;
	};
	FinalPlan plan;
	if (const int rc = final_plan(final_view(c), n_jobs, jobs, seqs_bytes, pos, cigars, n_ops, 1, long_min, tile_cols, set_err, measure, plan)) return rc;
	if (bound >= ((uint64_t)1 << 31)) return set_err(WM_ENOMEM, "batch can write 2^31 ops or more (its ops + its M columns = %llu); split it", (unsigned long long)bound);
	const std::vector<int> &order = plan.order;
	const std::vector<wm_final_pair> &tmap = plan.tmap;
	const size_t n_short = order.size(), n_tiles = tmap.size(), n_long = plan.lmap.size();
	wm_eqx_res_t *d_res = (wm_eqx_res_t*)arena_take(c, nj * sizeof(wm_eqx_res_t));
	int *d_cnt = (int*)arena_take(c, (nj * 3 + 16) * 4);
	int *d_total = (int*)arena_take(c, 64);
	int *d_part = (int*)arena_take(c, (n_tiles + 1) * 2 * 4);
	FinalDev V;
	const int staged = d_res && d_cnt && d_total && d_part ? final_stage(c, plan, cigars, n_ops, seqs, seqs_bytes, pos, 5, &V) : WM_ENOMEM;
	if (staged == WM_ENOMEM)
		return set_err(WM_ENOMEM, "eqx batch (%zu ops, %zu tiles, %zu sequence bytes) does not fit the arena of %.1f MB; split it", n_ops, n_tiles, pos ? (size_t)0 : seqs_bytes, c->arena_bytes / 1048576.0);
	if (staged) return staged;
	const wm_extra_djob_t *d_jobs = V.jobs;
	const size_t ps = V.pre_stride;
	const eqx_dev_pre P = { V.cig, V.pre, V.pre + ps, V.pre + 2 * ps, V.pre + 3 * ps, V.pre + 4 * ps };
	const final_dev_src D = { V.seqs, c->d_reads, c->d_reads_nm, c->d_S };
	// ---- count ----
	hipLaunchKernelGGL(eqx_prefix_kernel, dim3(n_jobs), dim3(64), 0, c->stream, d_jobs, P);
	if (n_short) {
		if (pos) hipLaunchKernelGGL(eqx_short_count_kernel<true>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, V.order, D, P, tile_cols, d_cnt);
		else hipLaunchKernelGGL(eqx_short_count_kernel<false>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, V.order, D, P, tile_cols, d_cnt);
	}
	if (n_tiles) {
		if (pos) hipLaunchKernelGGL(eqx_tile_count_kernel<true>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, V.tmap, D, P, tile_cols, d_part);
		else hipLaunchKernelGGL(eqx_tile_count_kernel<false>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, V.tmap, D, P, tile_cols, d_part);
		hipLaunchKernelGGL(eqx_combine_kernel, dim3((unsigned)n_long), dim3(64), 0, c->stream, d_jobs, V.lmap, P, d_part, d_cnt);
	}
	hipLaunchKernelGGL(eqx_job_scan_kernel, dim3(1), dim3(64), 0, c->stream, d_cnt, n_jobs, d_res, d_total);
	HIPCHK(hipGetLastError());
	std::vector<wm_eqx_res_t> res(nj);                                 // (out[] stays untouched when the arena refuses the write pass: a refused batch is split and issued again)
	HIPCHK(hipMemcpyAsync(res.data(), d_res, nj * sizeof(wm_eqx_res_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));
	const size_t total = (size_t)res[nj - 1].off + (size_t)res[nj - 1].n_cigar;
	*out_used = total;
	if (total > bound) return set_err(WM_ENODEV, "internal: the count pass reports %zu ops, more than the %llu the batch can have", total, (unsigned long long)bound);
	if (total > out_cap) { memcpy(out, res.data(), nj * sizeof(wm_eqx_res_t)); return set_err(WM_ENOMEM, "cigars_out holds %zu ops, the batch needs %zu", out_cap, total); }
	if (total == 0) { memcpy(out, res.data(), nj * sizeof(wm_eqx_res_t)); return WM_OK; }
	// ---- write: the jobs of the rewrite branch walk their columns again; then every job's ops ----
	uint32_t *d_out = (uint32_t*)arena_take(c, (total + 16) * 4);
	std::vector<int> order2; std::vector<wm_final_pair> tmap2;
	for (size_t g = 0; g < n_short; ++g) if (!res[order[g]].in_place && mcols[order[g]] > 0) order2.push_back(order[g]);
	for (size_t g = 0; g < n_tiles; ++g) if (!res[tmap[g].x].in_place) tmap2.push_back(tmap[g]);
	int *d_order2 = (int*)arena_take(c, (order2.size() + 16) * 4);
	int2 *d_tmap2 = (int2*)arena_take(c, (tmap2.size() + 16) * sizeof(int2));
	if (!d_out || !d_order2 || !d_tmap2)
		return set_err(WM_ENOMEM, "eqx batch (%zu ops out) does not fit the arena of %.1f MB; split it", total, c->arena_bytes / 1048576.0);
	memcpy(out, res.data(), nj * sizeof(wm_eqx_res_t));
	if (!order2.empty()) {
		HIPCHK(hipMemcpyAsync(d_order2, order2.data(), order2.size() * 4, hipMemcpyHostToDevice, c->stream));
		if (pos) hipLaunchKernelGGL(eqx_short_write_kernel<true>, dim3((unsigned)order2.size()), dim3(64), 0, c->stream, d_jobs, d_order2, D, P, tile_cols, d_res, d_out);
		else hipLaunchKernelGGL(eqx_short_write_kernel<false>, dim3((unsigned)order2.size()), dim3(64), 0, c->stream, d_jobs, d_order2, D, P, tile_cols, d_res, d_out);
	}
	if (!tmap2.empty()) {
		HIPCHK(hipMemcpyAsync(d_tmap2, tmap2.data(), tmap2.size() * sizeof(int2), hipMemcpyHostToDevice, c->stream));
		if (pos) hipLaunchKernelGGL(eqx_tile_write_kernel<true>, dim3((unsigned)tmap2.size()), dim3(64), 0, c->stream, d_jobs, d_tmap2, D, P, tile_cols, d_part, d_res, d_out);
		else hipLaunchKernelGGL(eqx_tile_write_kernel<false>, dim3((unsigned)tmap2.size()), dim3(64), 0, c->stream, d_jobs, d_tmap2, D, P, tile_cols, d_part, d_res, d_out);
	}
	hipLaunchKernelGGL(eqx_ops_kernel, dim3(n_jobs), dim3(64), 0, c->stream, d_jobs, P, d_res, d_out);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(cigars_out, d_out, total * 4, hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));                     // (order2 / tmap2 are pageable: they stay alive until the stream has taken them)
	return WM_OK;
}
catch (const std::bad_alloc &) { return set_err(WM_ENOMEM, "out of host memory"); }

// mm_update_cigar_eqx (src/align.c:169-238) over final CIGARs, operands as 0..4 codes inside seqs
extern "C" int wm_eqx_batch(wm_ctx_t *c, int n_jobs, const wm_extra_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes, const uint32_t *cigars, size_t n_ops,
                            uint32_t *cigars_out, size_t out_cap, size_t *out_used, wm_eqx_res_t *out)
{
	if (n_jobs > 0 && !jobs) return set_err(WM_EINVAL, "null jobs");
	return eqx_batch_impl(c, n_jobs, jobs, seqs, seqs_bytes, 0, cigars, n_ops, cigars_out, out_cap, out_used, out);
}
// mm_update_cigar_eqx (src/align.c:169-238) over final CIGARs, operands as positions in the resident reads (two-strand space) and the uploaded reference
extern "C" int wm_eqx_batch_pos(wm_ctx_t *c, int n_jobs, const wm_extra_pos_t *jobs, const uint32_t *cigars, size_t n_ops,
                                uint32_t *cigars_out, size_t out_cap, size_t *out_used, wm_eqx_res_t *out)
{
	if (n_jobs > 0 && !jobs) return set_err(WM_EINVAL, "null jobs");
	return eqx_batch_impl(c, n_jobs, 0, 0, 0, jobs, cigars, n_ops, cigars_out, out_cap, out_used, out);
}

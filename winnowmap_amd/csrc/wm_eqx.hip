// wm_eqx.hip — libwmgpu.so, = / X unit: mm_update_cigar_eqx (src/align.c:169-238, the tail of mm_update_extra under MM_F_EQX, :285) over batches of regions' final
// CIGARs — wm_eqx_batch, wm_eqx_batch_pos of include/wm_gpu.h. The fold, the two passes and the slot arithmetic are in eqx_kernel.h, the specification in cigar_eqx.h;
// here are the kernel entry points, validation (the rules of wm_extra.hip), the split into the two classes by the values of wm_extra_set_routing, and the launches.
// (The mapper's switch and its counters live with the host mapper: host/wm_ops.cpp.)
#include "wm_rt.h"
#include "simt.h"
#include "eqx_kernel.h"

int extra_long_min_cols();          // wm_extra.hip

// ======================================================================================================
// kernels (one wavefront per workgroup)
// ======================================================================================================
struct eqx_dev_src { const uint8_t *seqs; const uint64_t *pk, *nm; const uint32_t *S; };
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
__global__ __launch_bounds__(64) void eqx_short_count_kernel(const wm_extra_djob_t *__restrict__ jobs, const int *__restrict__ order, eqx_dev_src D, eqx_dev_pre P, int tile_cols, int *cnt)
{
	const int j = order[blockIdx.x];
	EQX_JOB(j);
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::eqx_short_count(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, cnt + (size_t)j * 3);
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::eqx_short_count(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, cnt + (size_t)j * 3);
	}
}
// count, long class: workgroup g folds tile tmap[g].y of job tmap[g].x into part[2 g ..]; then one workgroup per long job turns its tiles' tuples into carries
template <bool POS>
__global__ __launch_bounds__(64) void eqx_tile_count_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ tmap, eqx_dev_src D, eqx_dev_pre P, int tile_cols, int *part)
{
	const int2 tm = tmap[blockIdx.x];
	EQX_JOB(tm.x);
	int *out = part + (size_t)blockIdx.x * 2;
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::eqx_long_count(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, tm.y, out);
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::eqx_long_count(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, tm.y, out);
	}
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
__global__ __launch_bounds__(64) void eqx_short_write_kernel(const wm_extra_djob_t *__restrict__ jobs, const int *__restrict__ order, eqx_dev_src D, eqx_dev_pre P, int tile_cols,
                                                              const wm_eqx_res_t *__restrict__ res, uint32_t *out)
{
	const int j = order[blockIdx.x];
	EQX_JOB(j);
	uint32_t *o = out + res[j].off;
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::eqx_short_write(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, o, gS);
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::eqx_short_write(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, o, gS);
	}
}
template <bool POS>
__global__ __launch_bounds__(64) void eqx_tile_write_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ tmap, eqx_dev_src D, eqx_dev_pre P, int tile_cols,
                                                             const int *__restrict__ part, const wm_eqx_res_t *__restrict__ res, uint32_t *out)
{
	const int2 tm = tmap[blockIdx.x];                          // (the tiles of the rewrite-branch jobs only: { job, tile })
	EQX_JOB(tm.x);
	uint32_t *o = out + res[tm.x].off;
	const int *pt = part + ((size_t)jb.tile0 + (size_t)tm.y) * 2;
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::eqx_long_write(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, tm.y, pt, o, gS);
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::eqx_long_write(S, cig, mS, qS, tS, cS, jb.n_cigar, tile_cols, tm.y, pt, o, gS);
	}
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
	std::vector<wm_extra_djob_t> dj(nj);
	std::vector<int64_t> mcols(nj);
	std::vector<int> order; std::vector<int2> tmap, lmap;
	size_t n_pre = 0;
	uint64_t bound = 0;                            // ops the call can write at most: every op, and one more per M column
	for (int i = 0; i < n_jobs; ++i) {
		const uint32_t cig_off = pos ? pos[i].cig_off : jobs[i].cig_off;
		const int32_t nc = pos ? pos[i].n_cigar : jobs[i].n_cigar;
		if (nc < 0 || (uint64_t)cig_off + (uint64_t)nc > n_ops) return set_err(WM_EINVAL, "job %d: CIGAR ops [%u, %u + %d) outside the %zu ops of the call", i, cig_off, cig_off, nc, n_ops);
		const wm_extra_measure_t ms = wm_extra_measure(cigars + cig_off, nc, &sc0);
		int64_t m = 0;
		for (int k = 0; k < nc; ++k) if ((cigars[cig_off + k] & 0xf) == 0) m += cigars[cig_off + k] >> 4;
		if (m >= ((int64_t)1 << 31) - 64 * (int64_t)tile_cols || ms.qlen >= ((int64_t)1 << 31) || ms.tlen >= ((int64_t)1 << 31))
			return set_err(WM_EINVAL, "job %d: the CIGAR spans 2^31 bases or more", i);
		mcols[i] = m;
		bound += (uint64_t)nc + (uint64_t)m;
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
		if (m > 0 && m >= long_min) {
			const int nt = (int)((m + tile_cols - 1) / tile_cols);
			if (tmap.size() + (size_t)nt >= ((size_t)1 << 28)) return set_err(WM_ENOMEM, "batch holds more than 2^28 tiles; split it");
			d.tile0 = (int32_t)tmap.size();
			for (int t = 0; t < nt; ++t) tmap.push_back(make_int2(i, t));
			lmap.push_back(make_int2(i, nt));
		} else order.push_back(i);
	}
	if (bound >= ((uint64_t)1 << 31)) return set_err(WM_ENOMEM, "batch can write 2^31 ops or more (its ops + its M columns = %llu); split it", (unsigned long long)bound);
	const size_t n_short = order.size(), n_tiles = tmap.size(), n_long = lmap.size();
	wm_extra_djob_t *d_jobs = (wm_extra_djob_t*)arena_take(c, nj * sizeof(wm_extra_djob_t));
	wm_eqx_res_t *d_res = (wm_eqx_res_t*)arena_take(c, nj * sizeof(wm_eqx_res_t));
	int *d_cnt = (int*)arena_take(c, (nj * 3 + 16) * 4);
	int *d_total = (int*)arena_take(c, 64);
	uint32_t *d_cig = (uint32_t*)arena_take(c, (n_ops + 16) * 4);
	int *d_pre = (int*)arena_take(c, 5 * (n_pre + 16) * 4);
	int *d_order = (int*)arena_take(c, (n_short + 16) * 4);
	int2 *d_tmap = (int2*)arena_take(c, (n_tiles + n_long + 16) * sizeof(int2));
	int *d_part = (int*)arena_take(c, (n_tiles + 1) * 2 * 4);
	uint8_t *d_seqs = pos ? 0 : (uint8_t*)arena_take(c, seqs_bytes + 64);
	if (!d_jobs || !d_res || !d_cnt || !d_total || !d_cig || !d_pre || !d_order || !d_tmap || !d_part || (!pos && !d_seqs))
		return set_err(WM_ENOMEM, "eqx batch (%zu ops, %zu tiles, %zu sequence bytes) does not fit the arena of %.1f MB; split it", n_ops, n_tiles, pos ? (size_t)0 : seqs_bytes, c->arena_bytes / 1048576.0);
	HIPCHK(hipMemcpyAsync(d_jobs, dj.data(), nj * sizeof(wm_extra_djob_t), hipMemcpyHostToDevice, c->stream));
	if (n_ops) HIPCHK(hipMemcpyAsync(d_cig, cigars, n_ops * 4, hipMemcpyHostToDevice, c->stream));
	if (n_short) HIPCHK(hipMemcpyAsync(d_order, order.data(), n_short * 4, hipMemcpyHostToDevice, c->stream));
	if (n_tiles) HIPCHK(hipMemcpyAsync(d_tmap, tmap.data(), n_tiles * sizeof(int2), hipMemcpyHostToDevice, c->stream));
	if (n_long) HIPCHK(hipMemcpyAsync(d_tmap + n_tiles, lmap.data(), n_long * sizeof(int2), hipMemcpyHostToDevice, c->stream));
	if (!pos && seqs_bytes) {
		HIPCHK(hipMemcpyAsync(d_seqs, seqs, seqs_bytes, hipMemcpyHostToDevice, c->stream));
		HIPCHK(hipMemsetAsync(d_seqs + seqs_bytes, 4, 64, c->stream));
	}
	const size_t ps = n_pre + 16;
	const eqx_dev_pre P = { d_cig, d_pre, d_pre + ps, d_pre + 2 * ps, d_pre + 3 * ps, d_pre + 4 * ps };
	const eqx_dev_src D = { d_seqs, c->d_reads, c->d_reads_nm, c->d_S };
	// ---- count ----
	hipLaunchKernelGGL(eqx_prefix_kernel, dim3(n_jobs), dim3(64), 0, c->stream, d_jobs, P);
	if (n_short) {
		if (pos) hipLaunchKernelGGL(eqx_short_count_kernel<true>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, d_order, D, P, tile_cols, d_cnt);
		else hipLaunchKernelGGL(eqx_short_count_kernel<false>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, d_order, D, P, tile_cols, d_cnt);
	}
	if (n_tiles) {
		if (pos) hipLaunchKernelGGL(eqx_tile_count_kernel<true>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, d_tmap, D, P, tile_cols, d_part);
		else hipLaunchKernelGGL(eqx_tile_count_kernel<false>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, d_tmap, D, P, tile_cols, d_part);
		hipLaunchKernelGGL(eqx_combine_kernel, dim3((unsigned)n_long), dim3(64), 0, c->stream, d_jobs, d_tmap + n_tiles, P, d_part, d_cnt);
	}
	hipLaunchKernelGGL(eqx_job_scan_kernel, dim3(1), dim3(64), 0, c->stream, d_cnt, n_jobs, d_res, d_total);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, d_res, nj * sizeof(wm_eqx_res_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));
	const size_t total = (size_t)out[nj - 1].off + (size_t)out[nj - 1].n_cigar;
	*out_used = total;
	if (total > bound) return set_err(WM_ENODEV, "internal: the count pass reports %zu ops, more than the %llu the batch can have", total, (unsigned long long)bound);
	if (total > out_cap) return set_err(WM_ENOMEM, "cigars_out holds %zu ops, the batch needs %zu", out_cap, total);
	if (total == 0) return WM_OK;
	// ---- write: the jobs of the rewrite branch walk their columns again; then every job's ops ----
	uint32_t *d_out = (uint32_t*)arena_take(c, (total + 16) * 4);
	std::vector<int> order2; std::vector<int2> tmap2;
	for (size_t g = 0; g < n_short; ++g) if (!out[order[g]].in_place && mcols[order[g]] > 0) order2.push_back(order[g]);
	for (size_t g = 0; g < n_tiles; ++g) if (!out[tmap[g].x].in_place) tmap2.push_back(tmap[g]);
	int *d_order2 = (int*)arena_take(c, (order2.size() + 16) * 4);
	int2 *d_tmap2 = (int2*)arena_take(c, (tmap2.size() + 16) * sizeof(int2));
	if (!d_out || !d_order2 || !d_tmap2)
		return set_err(WM_ENOMEM, "eqx batch (%zu ops out) does not fit the arena of %.1f MB; split it", total, c->arena_bytes / 1048576.0);
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

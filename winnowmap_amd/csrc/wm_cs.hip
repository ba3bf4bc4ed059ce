// wm_cs.hip — libwmgpu.so, cs / MD unit: the bodies of the cs:Z / MD:Z tags (write_cs_core, write_MD_core, src/format.c:141-218, under --cs, --cs=long, --MD) over
// batches of regions' final CIGARs — wm_cs_batch, wm_cs_batch_pos of include/wm_gpu.h. The column space, the fold and the two passes are in cs_kernel.h, the
// specification in cigar_cs.h; here are the kernel entry points, validation (the rules of wm_eqx.hip, and what the reference asserts), the split into the two
// classes by the values of wm_extra_set_routing, and the launches. (The mapper's switch and its counters live with the host mapper: host/wm_ops.cpp.)
#include "wm_rt.h"
#include "simt.h"
#include "cs_kernel.h"

int extra_long_min_cols();          // wm_extra.hip

// ======================================================================================================
// kernels (one wavefront per workgroup)
// ======================================================================================================
struct cs_dev_src { const uint8_t *seqs; const uint64_t *pk, *nm; const uint32_t *S; };
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
__global__ __launch_bounds__(64) void cs_short_count_kernel(const wm_extra_djob_t *__restrict__ jobs, const int *__restrict__ order, cs_dev_src D, cs_dev_pre P, int mode, int tile_cols, int *cnt)
{
	const int j = order[blockIdx.x];
	CS_JOB(j);
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::cs_short_count(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, cnt + j);
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::cs_short_count(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, cnt + j);
	}
}
// count, long class: workgroup g folds tile tmap[g].y of job tmap[g].x into part[4 g ..]; then one workgroup per long job turns its tiles' summaries into carries
template <bool POS>
__global__ __launch_bounds__(64) void cs_tile_count_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ tmap, cs_dev_src D, cs_dev_pre P, int mode, int tile_cols, int *part)
{
	const int2 tm = tmap[blockIdx.x];
	CS_JOB(tm.x);
	int *out = part + (size_t)blockIdx.x * 4;
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::cs_long_count(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, tm.y, out);
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::cs_long_count(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, tm.y, out);
	}
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
__global__ __launch_bounds__(64) void cs_short_write_kernel(const wm_extra_djob_t *__restrict__ jobs, const int *__restrict__ order, cs_dev_src D, cs_dev_pre P, int mode, int tile_cols,
                                                             const wm_cs_res_t *__restrict__ res, uint8_t *out)
{
	const int j = order[blockIdx.x];
	CS_JOB(j);
	uint8_t *o = out + res[j].off;
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::cs_short_write(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, o);
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::cs_short_write(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, o);
	}
}
template <bool POS>
__global__ __launch_bounds__(64) void cs_tile_write_kernel(const wm_extra_djob_t *__restrict__ jobs, const int2 *__restrict__ tmap, cs_dev_src D, cs_dev_pre P, int mode, int tile_cols,
                                                            const int *__restrict__ part, const wm_cs_res_t *__restrict__ res, uint8_t *out)
{
	const int2 tm = tmap[blockIdx.x];
	CS_JOB(tm.x);
	uint8_t *o = out + res[tm.x].off;
	const int *pt = part + (size_t)blockIdx.x * 4;
	if constexpr (POS) {
		const wmk::extra_src_pos S = { D.pk, D.nm, D.S, jb.q_base, jb.t_base, jb.q_pos, jb.q_len };
		wmk::cs_long_write(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, tm.y, pt, o);
	} else {
		const wmk::extra_src_bytes S = { D.seqs, jb.q_base, jb.t_base };
		wmk::cs_long_write(S, mode, cS, qS, tS, wS, jb.n_cigar, tile_cols, tm.y, pt, o);
	}
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
	std::vector<wm_extra_djob_t> dj(nj);
	std::vector<int> order; std::vector<int2> tmap, lmap;
	size_t n_pre = 0;
	uint64_t bound_all = 0;
	for (int i = 0; i < n_jobs; ++i) {
		const uint32_t cig_off = pos ? pos[i].cig_off : jobs[i].cig_off;
		const int32_t nc = pos ? pos[i].n_cigar : jobs[i].n_cigar;
		if (nc < 0 || (uint64_t)cig_off + (uint64_t)nc > n_ops) return set_err(WM_EINVAL, "job %d: CIGAR ops [%u, %u + %d) outside the %zu ops of the call", i, cig_off, cig_off, nc, n_ops);
		const uint32_t *cg = cigars + cig_off;
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
		wm_extra_djob_t &d = dj[i];
		memset(&d, 0, sizeof(d));
		d.cig_off = cig_off; d.n_cigar = nc; d.pre_off = (uint32_t)n_pre;
		n_pre += (size_t)nc + 2;
		if (n_pre >= ((size_t)1 << 31)) return set_err(WM_ENOMEM, "batch holds 2^31 CIGAR ops or more; split it");
		if (pos) {
			const wm_extra_pos_t &s = pos[i];
			if (nc > 0) {
				if (s.qwin_off < 0 || s.qwin_len < 0 || s.qwin_len >= (1 << 30) || (uint64_t)s.qwin_off + (uint64_t)s.qwin_len > c->reads_bytes)
					return set_err(WM_EINVAL, "job %d: the (sub)read lies outside the resident reads", i);
				if ((int64_t)s.q_pos < -16 || (int64_t)s.q_pos + qlen > 2 * (int64_t)s.qwin_len + 16)
					return set_err(WM_EINVAL, "job %d: the CIGAR consumes %lld query bases from two-strand position %d of a read of %d bases", i, (long long)qlen, s.q_pos, s.qwin_len);
				if (s.rid < 0 || (size_t)s.rid >= c->seq_len.size() || s.t_pos < 0 || (int64_t)s.t_pos + tlen > (int64_t)c->seq_len[s.rid])
					return set_err(WM_EINVAL, "job %d: the CIGAR consumes %lld target bases from base %d of contig %d", i, (long long)tlen, s.t_pos, s.rid);
				d.q_base = s.qwin_off; d.q_pos = s.q_pos; d.q_len = s.qwin_len; d.t_base = (long long)c->seq_off[s.rid] + s.t_pos;
			}
		} else {
			const wm_extra_job_t &s = jobs[i];
			if (nc > 0 && ((uint64_t)s.q_off + (uint64_t)qlen > seqs_bytes || (uint64_t)s.t_off + (uint64_t)tlen > seqs_bytes))
				return set_err(WM_EINVAL, "job %d: the CIGAR consumes %lld query / %lld target bases, more than seqs holds behind its offsets", i, (long long)qlen, (long long)tlen);
			d.q_base = s.q_off; d.t_base = s.t_off;
		}
		if (cols >= long_min) {
			const int nt = (int)((cols + tile_cols - 1) / tile_cols);
			if (tmap.size() + (size_t)nt >= ((size_t)1 << 28)) return set_err(WM_ENOMEM, "batch holds more than 2^28 tiles; split it");
			d.tile0 = (int32_t)tmap.size();
			for (int t = 0; t < nt; ++t) tmap.push_back(make_int2(i, t));
			lmap.push_back(make_int2(i, nt));
		} else order.push_back(i);
	}
	const size_t n_short = order.size(), n_tiles = tmap.size(), n_long = lmap.size();
	wm_extra_djob_t *d_jobs = (wm_extra_djob_t*)arena_take(c, nj * sizeof(wm_extra_djob_t));
	wm_cs_res_t *d_res = (wm_cs_res_t*)arena_take(c, nj * sizeof(wm_cs_res_t));
	int *d_cnt = (int*)arena_take(c, (nj + 16) * 4);
	int *d_total = (int*)arena_take(c, 64);
	uint32_t *d_cig = (uint32_t*)arena_take(c, (n_ops + 16) * 4);
	int *d_pre = (int*)arena_take(c, 4 * (n_pre + 16) * 4);
	int *d_order = (int*)arena_take(c, (n_short + 16) * 4);
	int2 *d_tmap = (int2*)arena_take(c, (n_tiles + n_long + 16) * sizeof(int2));
	int *d_part = (int*)arena_take(c, (n_tiles + 1) * 4 * 4);
	uint8_t *d_seqs = pos ? 0 : (uint8_t*)arena_take(c, seqs_bytes + 64);
	if (!d_jobs || !d_res || !d_cnt || !d_total || !d_cig || !d_pre || !d_order || !d_tmap || !d_part || (!pos && !d_seqs))
		return set_err(WM_ENOMEM, "cs batch (%zu ops, %zu tiles, %zu sequence bytes) does not fit the arena of %.1f MB; split it", n_ops, n_tiles, pos ? (size_t)0 : seqs_bytes, c->arena_bytes / 1048576.0);
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
	const cs_dev_pre P = { d_cig, d_pre, d_pre + ps, d_pre + 2 * ps, d_pre + 3 * ps };
	const cs_dev_src D = { d_seqs, c->d_reads, c->d_reads_nm, c->d_S };
	// ---- count ----
	hipLaunchKernelGGL(cs_prefix_kernel, dim3(n_jobs), dim3(64), 0, c->stream, d_jobs, P, mode);
	if (n_short) {
		if (pos) hipLaunchKernelGGL(cs_short_count_kernel<true>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, d_order, D, P, mode, tile_cols, d_cnt);
		else hipLaunchKernelGGL(cs_short_count_kernel<false>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, d_order, D, P, mode, tile_cols, d_cnt);
	}
	if (n_tiles) {
		if (pos) hipLaunchKernelGGL(cs_tile_count_kernel<true>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, d_tmap, D, P, mode, tile_cols, d_part);
		else hipLaunchKernelGGL(cs_tile_count_kernel<false>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, d_tmap, D, P, mode, tile_cols, d_part);
		hipLaunchKernelGGL(cs_combine_kernel, dim3((unsigned)n_long), dim3(64), 0, c->stream, d_jobs, d_tmap + n_tiles, d_part, d_cnt);
	}
	hipLaunchKernelGGL(cs_job_scan_kernel, dim3(1), dim3(64), 0, c->stream, d_cnt, n_jobs, d_res, d_total);
	HIPCHK(hipGetLastError());
	HIPCHK(hipMemcpyAsync(out, d_res, nj * sizeof(wm_cs_res_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));
	const uint64_t total = out[nj - 1].off + (uint64_t)out[nj - 1].len;
	*out_used = (size_t)total;
	if (total > bound_all) return set_err(WM_ENODEV, "internal: the count pass reports %llu bytes, more than the %llu the batch can have", (unsigned long long)total, (unsigned long long)bound_all);
	if (total > out_cap) return set_err(WM_ENOMEM, "text_out holds %zu bytes, the batch needs %llu", out_cap, (unsigned long long)total);
	if (total == 0) return WM_OK;
	// ---- write: every job walks its columns again, every lane from its own byte offset ----
	uint8_t *d_out = (uint8_t*)arena_take(c, (size_t)total + 64);
	if (!d_out) return set_err(WM_ENOMEM, "cs batch (%llu bytes out) does not fit the arena of %.1f MB; split it", (unsigned long long)total, c->arena_bytes / 1048576.0);
	if (n_short) {
		if (pos) hipLaunchKernelGGL(cs_short_write_kernel<true>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, d_order, D, P, mode, tile_cols, d_res, d_out);
		else hipLaunchKernelGGL(cs_short_write_kernel<false>, dim3((unsigned)n_short), dim3(64), 0, c->stream, d_jobs, d_order, D, P, mode, tile_cols, d_res, d_out);
	}
	if (n_tiles) {
		if (pos) hipLaunchKernelGGL(cs_tile_write_kernel<true>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, d_tmap, D, P, mode, tile_cols, d_part, d_res, d_out);
		else hipLaunchKernelGGL(cs_tile_write_kernel<false>, dim3((unsigned)n_tiles), dim3(64), 0, c->stream, d_jobs, d_tmap, D, P, mode, tile_cols, d_part, d_res, d_out);
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

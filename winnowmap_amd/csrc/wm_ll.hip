// wm_ll.hip — libwmgpu.so, local-score unit: ksw_ll_qinit + ksw_ll_i16 (src/ksw2.h:82-83, src/ksw2_ll_sse.c:32-147) over batches of jobs — wm_ksw_ll_batch,
// wm_ksw_ll_batch_pos of include/wm_gpu.h. The machine is in ll_kernel.h, the specification in ksw_ll.h; here are the kernel entry points, what the call refuses, the
// split into the size classes and the launches. (The mapper's switch and its counters live with the host mapper: host/wm_ops.cpp.)
#include "wm_rt.h"
#include "simt.h"
#include "ll_kernel.h"

// ======================================================================================================
// kernels (one wavefront per workgroup, one workgroup per job)
// ======================================================================================================
struct ll_djob { long long qb, tb; int q_pos, L, qlen, tlen, step, pad; };      // bytes: qb / tb = element 0 in the slab; positions: qb = qwin_off, tb = element 0 in the packed reference
struct ll_dev_src { const uint8_t *seqs; const uint64_t *pk, *nm; const uint32_t *S; };

// ROWS = 0: the register class; otherwise the LDS class for targets of at most ROWS rows (two ints per row)
template <bool POS, int ROWS>
__global__ __launch_bounds__(64) void ll_kernel(const ll_djob *__restrict__ jobs, const int *__restrict__ order, ll_dev_src D, const int *__restrict__ mat, int oe, int ext, int *out)
{
	__shared__ int rows[ROWS ? 2 * ROWS : 1];
	const int j = order[blockIdx.x];
	const ll_djob jb = jobs[j];
	if (ROWS && jb.tlen > ROWS) return;                        // (the host never routes such a job here)
	if constexpr (POS) {
		const wmk::ll_src_pos S = { D.pk, D.nm, D.S, jb.qb, jb.tb, jb.q_pos, jb.L, jb.step };
		wmk::ll_job<ROWS != 0>(S, jb.qlen, jb.tlen, mat, oe, ext, rows, out + (size_t)3 * j);
	} else {
		const wmk::ll_src_bytes S = { D.seqs, jb.qb, jb.tb, jb.step };
		wmk::ll_job<ROWS != 0>(S, jb.qlen, jb.tlen, mat, oe, ext, rows, out + (size_t)3 * j);
	}
}

// ======================================================================================================
// routing
// ======================================================================================================
enum { LL_ROWS_MID = 8192 };                                   // 64 KB of LDS; longer targets take the WM_LL_MAX_LEN-row instantiation (128 KB: one workgroup per CU)
static_assert(WM_LL_MAX_LEN > LL_ROWS_MID && 2 * 4 * WM_LL_MAX_LEN <= 160 * 1024, "the big LDS class holds WM_LL_MAX_LEN rows in a CU's 160 KB");
static std::atomic<int> g_ll_reg_max(64);
extern "C" void wm_ksw_ll_set_routing(int reg_max) { if (reg_max >= 0 && reg_max <= 64) g_ll_reg_max = reg_max; }
extern "C" int wm_ksw_ll_reg_max(void) { return g_ll_reg_max.load(); }

template <bool POS>
static void ll_launch(wm_ctx_t *c, int klass, unsigned n, const ll_djob *jobs, const int *order, const ll_dev_src &D, const int *mat, int oe, int ext, int *out)
{
	if (klass == 0) hipLaunchKernelGGL((ll_kernel<POS, 0>), dim3(n), dim3(64), 0, c->stream, jobs, order, D, mat, oe, ext, out);
	else if (klass == 1) hipLaunchKernelGGL((ll_kernel<POS, LL_ROWS_MID>), dim3(n), dim3(64), 0, c->stream, jobs, order, D, mat, oe, ext, out);
	else hipLaunchKernelGGL((ll_kernel<POS, WM_LL_MAX_LEN>), dim3(n), dim3(64), 0, c->stream, jobs, order, D, mat, oe, ext, out);
}

// ======================================================================================================
// the batched call
// ======================================================================================================
static int ll_batch_impl(wm_ctx_t *c, const int8_t *mat, int gapo, int gape, int n_jobs, const wm_ll_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes, const wm_ll_pos_t *pos, wm_ll_res_t *out)
try {
	if (!c) return set_err(WM_EINVAL, "null context");
	if (n_jobs < 0) return set_err(WM_EINVAL, "n_jobs < 0");
	if (gapo <= 0 || gape <= 0) return set_err(WM_EINVAL, "gapo = %d, gape = %d: both must be positive (with gapo = 0 the striped reference drops F values that tie)", gapo, gape);
	if ((int64_t)gapo + gape > 32767) return set_err(WM_EINVAL, "gapo + gape = %lld does not fit the reference's int16 lanes", (long long)gapo + gape);
	if (n_jobs == 0) return WM_OK;
	if (!mat || !out || (!jobs && !pos) || (jobs && seqs_bytes && !seqs)) return set_err(WM_EINVAL, "null argument");
	if (pos && (!c->d_S || c->seq_len.empty())) return set_err(WM_EINVAL, "position jobs need wm_index_upload on this context");
	if (pos && !c->d_reads) return set_err(WM_EINVAL, "position jobs need wm_reads_upload on this context");
	const size_t nj = (size_t)n_jobs;
	const int reg_max = g_ll_reg_max.load();
	std::vector<ll_djob> dj(nj);
	std::vector<int> order[3];
	size_t lo = seqs_bytes, hi = 0;
	for (int i = 0; i < n_jobs; ++i) {
		const int qlen = pos ? pos[i].qlen : jobs[i].qlen, tlen = pos ? pos[i].tlen : jobs[i].tlen, step = pos ? pos[i].step : jobs[i].step;
		if (qlen < 1 || tlen < 1) return set_err(WM_EINVAL, "job %d: qlen = %d, tlen = %d (both must be at least 1)", i, qlen, tlen);
		if (qlen > WM_LL_MAX_LEN || tlen > WM_LL_MAX_LEN) return set_err(WM_EINVAL, "job %d: qlen = %d, tlen = %d exceed WM_LL_MAX_LEN = %d", i, qlen, tlen, WM_LL_MAX_LEN);
		if (step != 1 && step != -1) return set_err(WM_EINVAL, "job %d: step %d is neither 1 nor -1", i, step);
		ll_djob &d = dj[i];
		d.qlen = qlen; d.tlen = tlen; d.step = step; d.pad = 0;
		if (pos) {
			const wm_ll_pos_t &s = pos[i];
			const int64_t t_last = (int64_t)s.t_pos + (int64_t)(tlen - 1) * step;
			if (s.rid < 0 || (size_t)s.rid >= c->seq_len.size() || s.t_pos < 0 || t_last < 0 || (uint32_t)s.t_pos >= c->seq_len[s.rid] || (uint64_t)t_last >= c->seq_len[s.rid] ||
			    s.qwin_off < 0 || s.qwin_len < 0 || s.qwin_len >= (1 << 30) || s.q_pos <= -(1 << 30) || s.q_pos >= (1 << 30) ||
			    (uint64_t)s.qwin_off + (uint64_t)s.qwin_len > c->reads_bytes)
				return set_err(WM_EINVAL, "job %d: operand positions outside the resident reads / reference", i);
			d.qb = s.qwin_off; d.tb = (long long)c->seq_off[s.rid] + s.t_pos; d.q_pos = s.q_pos; d.L = s.qwin_len;
		} else {
			const wm_ll_job_t &s = jobs[i];
			if ((size_t)s.q_off + qlen > seqs_bytes || (size_t)s.t_off + tlen > seqs_bytes) return set_err(WM_EINVAL, "job %d: sequence offsets outside seqs", i);
			lo = std::min(lo, (size_t)std::min(s.q_off, s.t_off));
			hi = std::max(hi, std::max((size_t)s.q_off + qlen, (size_t)s.t_off + tlen));
			d.qb = step > 0 ? (long long)s.q_off : (long long)s.q_off + qlen - 1; d.tb = step > 0 ? (long long)s.t_off : (long long)s.t_off + tlen - 1; d.q_pos = 0; d.L = 0;
		}
		order[(qlen + 7) / 8 * 8 <= reg_max ? 0 : tlen <= LL_ROWS_MID ? 1 : 2].push_back(i);
	}
	if (!pos) for (ll_djob &d : dj) { d.qb -= (long long)lo; d.tb -= (long long)lo; }      // only [lo, hi) of the caller's buffer travels
	const size_t slab = pos ? 0 : hi - lo;
	HIPCHK(hipSetDevice(c->device));
	ArenaMark mark(c);
	ll_djob *d_jobs = (ll_djob*)arena_take(c, nj * sizeof(ll_djob));
	int *d_order = (int*)arena_take(c, (nj + 16) * 4);
	int *d_mat = (int*)arena_take(c, 32 * 4);
	int *d_out = (int*)arena_take(c, (nj * 3 + 16) * 4);
	uint8_t *d_seqs = pos ? 0 : (uint8_t*)arena_take(c, slab + 64);
	if (!d_jobs || !d_order || !d_mat || !d_out || (!pos && !d_seqs))
		return set_err(WM_ENOMEM, "ll batch (%d jobs, %zu sequence bytes) does not fit the arena of %.1f MB; split it", n_jobs, slab, c->arena_bytes / 1048576.0);
	int matw[32] = { 0 };
	for (int i = 0; i < 25; ++i) matw[i] = mat[i];
	std::vector<int> ord;
	ord.reserve(nj);
	for (const std::vector<int> &o : order) ord.insert(ord.end(), o.begin(), o.end());
	HIPCHK(hipMemcpyAsync(d_jobs, dj.data(), nj * sizeof(ll_djob), hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_order, ord.data(), nj * 4, hipMemcpyHostToDevice, c->stream));
	HIPCHK(hipMemcpyAsync(d_mat, matw, sizeof(matw), hipMemcpyHostToDevice, c->stream));
	if (slab) HIPCHK(hipMemcpyAsync(d_seqs, seqs + lo, slab, hipMemcpyHostToDevice, c->stream));
	const ll_dev_src D = { d_seqs, c->d_reads, c->d_reads_nm, c->d_S };
	size_t at = 0;
	for (int k = 0; k < 3; ++k) {
		const unsigned n = (unsigned)order[k].size();
		if (n) { if (pos) ll_launch<true>(c, k, n, d_jobs, d_order + at, D, d_mat, gapo + gape, gape, d_out); else ll_launch<false>(c, k, n, d_jobs, d_order + at, D, d_mat, gapo + gape, gape, d_out); }
		at += n;
	}
	HIPCHK(hipGetLastError());
	std::vector<wm_ll_res_t> res(nj);
	static_assert(sizeof(wm_ll_res_t) == 12, "wm_ll_res_t is the kernel's three ints");
	HIPCHK(hipMemcpyAsync(res.data(), d_out, nj * sizeof(wm_ll_res_t), hipMemcpyDeviceToHost, c->stream));
	HIPCHK(ctx_sync(c));
	memcpy(out, res.data(), nj * sizeof(wm_ll_res_t));                 // (out stays untouched unless the whole call succeeded)
	return WM_OK;
}
catch (const std::bad_alloc &) { return set_err(WM_ENOMEM, "out of host memory"); }

// ksw_ll_qinit + ksw_ll_i16 (src/ksw2.h:82-83), operands as 0..4 codes inside seqs
extern "C" int wm_ksw_ll_batch(wm_ctx_t *c, const int8_t *mat5x5, int gapo, int gape, int n_jobs, const wm_ll_job_t *jobs, const uint8_t *seqs, size_t seqs_bytes, wm_ll_res_t *out)
{
	if (n_jobs > 0 && !jobs) return set_err(WM_EINVAL, "null jobs");
	return ll_batch_impl(c, mat5x5, gapo, gape, n_jobs, jobs, seqs, seqs_bytes, 0, out);
}
// ksw_ll_qinit + ksw_ll_i16 (src/ksw2.h:82-83), operands as positions in the resident reads (two-strand space) and the uploaded reference
extern "C" int wm_ksw_ll_batch_pos(wm_ctx_t *c, const int8_t *mat5x5, int gapo, int gape, int n_jobs, const wm_ll_pos_t *jobs, wm_ll_res_t *out)
{
	if (n_jobs > 0 && !jobs) return set_err(WM_EINVAL, "null jobs");
	return ll_batch_impl(c, mat5x5, gapo, gape, n_jobs, 0, 0, 0, jobs, out);
}

// wm_mapper.hip — libwmgpu.so, mapper unit: the device contexts of a mapper as a pool shared by its mapping calls (GpuOps), wm_map_reads / wm_map_file* (the
// replacement of kt_for(worker_for) and mm_map_file, src/map.c:1008-1268), index parts, statistics. The host sources of the path (host/*.cpp: hit.c, align.c,
// map.c, format.c restated) are compiled in this unit.
#include "wm_rt.h"
#include "reads2bit.h"
#include <optional>
// ======================================================================================================
// sketch / seed / chain kernels and their batched entry points
// ======================================================================================================
#include "host/wm_core.cpp"
#include "host/wm_index.cpp"
#include "host/wm_seqio.cpp"
#include "host/wm_hit.cpp"
#include "host/wm_chain.cpp"
#include "host/wm_ops.cpp"
#include "host/wm_align.cpp"
#include "host/wm_mapper.cpp"
#include "host/wm_format.cpp"
#include "host/wm_kmers.cpp"
#include "host/wm_pipeline.cpp"

// process-wide account of splice mode's alignment calls (wm_exts2_stats): calls of GpuOpsCtx::exts2_batch that held requests, and the groups they were
// split into (one wm_ksw_exts2_batch each)
static std::atomic<uint64_t> g_exts2_calls{0}, g_exts2_groups{0};
extern "C" void wm_exts2_stats(uint64_t *out2, int reset)
{
	if (out2) { out2[0] = g_exts2_calls.load(); out2[1] = g_exts2_groups.load(); }
	if (reset) { g_exts2_calls = 0; g_exts2_groups = 0; }
}
// process-wide account of GpuOps::run_split (wm_arena_split_stats): batched calls (or parts of one) that were refused for the arena and halved, and the parts
// that were finally issued without being halved again
static std::atomic<uint64_t> g_split_halved{0}, g_split_parts{0};
extern "C" void wm_arena_split_stats(uint64_t *out2, int reset)
{
	if (out2) { out2[0] = g_split_halved.load(); out2[1] = g_split_parts.load(); }
	if (reset) { g_split_halved = 0; g_split_parts = 0; }
}

// ======================================================================================================
// GpuOps: the product implementation of the mapper's device operations
// ======================================================================================================
// the name keys of a request list (self / all-vs-all mapping): all requests of a call come from one mapper, so all or none carry one; empty = none
template <class R> static std::vector<wm_qkey_t> name_keys(const std::vector<R*> &reqs)
{
	std::vector<wm_qkey_t> keys;
	if (reqs[0]->has_key) { keys.resize(reqs.size()); for (size_t i = 0; i < reqs.size(); ++i) keys[i] = { reqs[i]->q_lo, reqs[i]->q_eq }; }
	return keys;
}

// one device context (stream + arena + staging slab) worth of batched operations; GpuOps below hands the contexts out
struct GpuOpsCtx {
	wm_ctx_t *c;
	uint64_t cells = 0;
	double ksw_us = 0, aux_us = 0;
	double t_pack = 0, t_prep = 0, t_run = 0, t_fetch = 0, t_unpack = 0, t_sketch = 0, t_seed = 0, t_chain = 0;
	std::string error;
	void fail(const char *what) { if (error.empty()) error = std::string(what) + ": " + wm_err_text(); }
	bool resident = false;                      // the mini-batch's read codes are on the device (load_reads)
	void sketch_batch(int, int, std::vector<wm::SketchReq*> &reqs)
	{
		const int n = (int)reqs.size();
		std::vector<uint64_t> off(n), ooff(n);
		std::vector<int32_t> len(n), cnt(n);
		std::vector<uint8_t> res(n, 0);
		size_t tot = 0, tot_all = 0;                // bytes to stage (sequences that are not resident); all bases
		for (int i = 0; i < n; ++i) {
			len[i] = reqs[i]->len; tot_all += reqs[i]->len;
			if (resident && reqs[i]->dev_off >= 0) { res[i] = 1; off[i] = (uint64_t)reqs[i]->dev_off; }
			else { off[i] = tot; tot += reqs[i]->len; }
		}
		UBuf<uint8_t> seqs(tot + 1, c);
		WM_SITE("sketch.stage");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) { if (!res[i]) memcpy(seqs.data() + off[i], reqs[i]->seq, reqs[i]->len); });
		UBuf<wm128_t> out(tot_all / 8 + (size_t)17 * n + 64, c);          // the batch tries len/8 + 16 slots per sequence first
		const double ts = now_ms();
		int rc = sketch_batch_impl(c, n, seqs.data(), tot, off.data(), len.data(), res.data(), out.data(), out.size(), ooff.data(), cnt.data());
		if (rc == WM_ENOMEM && strstr(wm_err_text(), "minimizer output pool")) {   // pathological density: redo with one slot per base
			UBuf<wm128_t> big(tot_all + n + 1);
			rc = sketch_batch_impl(c, n, seqs.data(), tot, off.data(), len.data(), res.data(), big.data(), big.size(), ooff.data(), cnt.data());
			if (rc) { fail("sketch"); return; }
			t_sketch += now_ms() - ts;
			aux_us += c->aux_ms * 1e3;
			wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) { reqs[i]->mini.assign(big.begin() + ooff[i], big.begin() + ooff[i] + cnt[i]); });
			return;
		}
		if (rc) { fail("sketch"); return; }
		t_sketch += now_ms() - ts;
		aux_us += c->aux_ms * 1e3;
		WM_SITE("sketch.unpack");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) { reqs[i]->mini.assign(out.begin() + ooff[i], out.begin() + ooff[i] + cnt[i]); });
	}
	void seed_batch(std::vector<wm::SeedReq*> &reqs)
	{
		const int n = (int)reqs.size();
		// one launch per (max_occ, flag) class; in practice a single class
		std::vector<uint64_t> moff(n), ooff(n);
		std::vector<int32_t> nm(n), ql(n), na(n), rl(n);
		size_t tot = 0;
		for (int i = 0; i < n; ++i) { moff[i] = tot; nm[i] = reqs[i]->n_mini; ql[i] = reqs[i]->qlen; tot += reqs[i]->n_mini; }
		const std::vector<wm_qkey_t> keys = name_keys(reqs);
		UBuf<wm128_t> mini(tot + 1, c);
		WM_SITE("seed.pack");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) { memcpy(mini.data() + moff[i], reqs[i]->mini, (size_t)reqs[i]->n_mini * sizeof(wm128_t)); });
		size_t cap = tot * 3 + 4096;               // anchors per minimizer: ~1.15 on the bench reference; repeats are retried at 8x
		for (int attempt = 0; attempt < 6; ++attempt) {
			UBuf<wm128_t> out(cap, c);
			const double ts = now_ms();
			const int rc = wm_seed_batch_keyed(c, n, mini.data(), moff.data(), nm.data(), ql.data(), keys.empty() ? 0 : keys.data(), reqs[0]->max_occ, reqs[0]->flag, out.data(), out.size(), ooff.data(), na.data(), rl.data());
			if (rc == WM_ENOMEM && strstr(wm_err_text(), "anchor output pool")) { cap *= 8; continue; }
			if (rc) { fail("seed"); return; }
			t_seed += now_ms() - ts;
			aux_us += c->aux_ms * 1e3;
			wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) { reqs[i]->a.assign(out.begin() + ooff[i], out.begin() + ooff[i] + na[i]); reqs[i]->rep_len = rl[i]; });
			return;
		}
		fail("seed (anchor pool)");
	}
	void chain_batch(std::vector<wm::ChainReq*> &reqs)
	{
		const int n = (int)reqs.size();
		std::vector<uint64_t> aoff(n), uoff(n);
		std::vector<int32_t> na(n), nu(n), nv(n);
		std::vector<wm_chain_par_t> par(n);
		size_t tot = 0;
		for (int i = 0; i < n; ++i) {
			aoff[i] = tot; na[i] = (int)reqs[i]->a.size(); tot += reqs[i]->a.size();
			par[i] = chain_par_of(*reqs[i]);
		}
		UBuf<wm128_t> a(tot + 1, c);
		UBuf<uint64_t> u(tot + 1, c);
		WM_SITE("chain.pack");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) { memcpy(a.data() + aoff[i], reqs[i]->a.data(), reqs[i]->a.size() * sizeof(wm128_t)); });
		const double ts = now_ms();
		if (wm_chain_batch(c, n, a.data(), aoff.data(), na.data(), par.data(), u.data(), uoff.data(), nu.data(), nv.data())) { fail("chain"); return; }
		t_chain += now_ms() - ts;
		aux_us += c->aux_ms * 1e3;
		WM_SITE("chain.unpack");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) {
			reqs[i]->u.assign(u.begin() + uoff[i], u.begin() + uoff[i] + nu[i]);
			reqs[i]->a.assign(a.begin() + aoff[i], a.begin() + aoff[i] + nv[i]);
		});
	}
	// the whole window on the device (wm_window_batch's machinery; the result pools are sized after the launch, in the pinned slab)
	void window_batch(std::vector<wm::WindowReq*> &reqs)
	{
		const int n = (int)reqs.size();
		if (n == 0) return;
		for (int i = 1; i < n; ++i)             // collect_seed_hits takes one (max_occ, flag), the -T filter one threshold per call: requests that differ go in their own call
			if (reqs[i]->max_occ != reqs[0]->max_occ || reqs[i]->flag != reqs[0]->flag || reqs[i]->sdust_thres != reqs[0]->sdust_thres) {
				std::vector<wm::WindowReq*> same, rest;
				for (wm::WindowReq *r : reqs) (r->max_occ == reqs[0]->max_occ && r->flag == reqs[0]->flag && r->sdust_thres == reqs[0]->sdust_thres ? same : rest).push_back(r);
				window_batch(same);
				if (error.empty()) window_batch(rest);
				return;
			}
		const double ts = now_ms();
		UBuf<wm_window_job_t> jobs(n, c);
		const std::vector<wm_qkey_t> keys = name_keys(reqs);
		size_t stage = 0, npre = 0;
		for (int i = 0; i < n; ++i) {
			const wm::WindowReq &r = *reqs[i];
			wm_window_job_t &j = jobs[i];
			j.len = r.len; j.n_pre = (int32_t)r.pre.size(); j.pre_off = npre; npre += r.pre.size();
			j.stage_off = 0;
			if (r.len <= 0) j.seq_off = -2;
			else if (resident && r.dev_off >= 0) j.seq_off = r.dev_off;
			else { j.seq_off = -1; j.stage_off = stage; stage += (size_t)r.len; }
			j.par = chain_par_of(r);
		}
		UBuf<uint8_t> seqs(stage + 1, c);
		UBuf<wm128_t> pre(npre + 1, c);
		UBuf<wm_window_res_t> res(n, c);
		WM_SITE("window.stage");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) {
			const wm::WindowReq &r = *reqs[i];
			if (jobs[i].seq_off == -1) memcpy(seqs.data() + jobs[i].stage_off, r.seq, (size_t)r.len);
			if (!r.pre.empty()) memcpy(pre.data() + jobs[i].pre_off, r.pre.data(), r.pre.size() * sizeof(wm128_t));
		});
		if (hipSetDevice(c->device) != hipSuccess) { error = "hipSetDevice failed"; return; }
		std::optional<UBuf<uint64_t>> up;           // the result pools: sized once the call knows its totals, in the pinned slab
		std::optional<UBuf<wm128_t>> ap;
		if (window_run(c, n, jobs.data(), keys.empty() ? 0 : keys.data(), seqs.data(), stage, pre.data(), npre, reqs[0]->max_occ, reqs[0]->flag, reqs[0]->sdust_thres, res.data(),
		               [&](uint32_t n_chains, uint32_t n_anchors, uint64_t **u_pool, wm128_t **a_pool) {
			up.emplace((size_t)n_chains + 1, c); ap.emplace((size_t)n_anchors + 1, c);
			*u_pool = up->data(); *a_pool = ap->data();
			return WM_OK;
		})) { fail("window"); return; }
		t_sketch += now_ms() - ts;
		aux_us += c->aux_ms * 1e3;
		WM_SITE("window.unpack");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) {
			wm::WindowReq &r = *reqs[i];
			const wm_window_res_t &o = res[i];
			r.rep_len = o.rep_len; r.n_anchors = o.n_anchors;
			r.u.assign(up->begin() + o.u_off, up->begin() + o.u_off + o.n_u);
			r.a.resize((size_t)o.n_v);
			if (o.n_v) memcpy(r.a.data(), ap->data() + o.a_off, (size_t)o.n_v * sizeof(wm128_t));
		});
	}
	void ksw_batch(const wm_ksw_score_t &sc, std::vector<wm::KswReq*> &reqs)
	{
		const double t0 = now_ms();
		const int n = (int)reqs.size();
		size_t cap = 16;
		bool all_res = resident;
		for (int i = 0; i < n && all_res; ++i) all_res = reqs[i]->resident();
		for (int i = 0; i < n; ++i) cap += (size_t)reqs[i]->ql + reqs[i]->tl + 2;
		std::vector<wm_ksw_result_t> res(n);
		std::vector<wm_zd_t> zd;
		UBuf<uint32_t> pool(cap, c);
		size_t used = 0;
		c->acc_cells = 0; c->t_prep = c->t_run = c->t_fetch = 0;
		double t1;
		if (all_res) {          // operands as positions in the resident reads / packed reference: nothing is copied or shipped per alignment
			UBuf<wm_ksw_pos_t> jobs(n + 1, c);
			WM_SITE("ksw.pos_jobs");
			wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) {
				const wm::KswReq &r = *reqs[i];
				wm_ksw_pos_t &j = jobs[i];
				j.qwin_off = r.qwin_off; j.qwin_len = r.qwin_len; j.q_pos = r.q_pos; j.rid = r.rid; j.t_pos = r.t_pos; j.qlen = r.ql; j.tlen = r.tl;
				j.w = r.w; j.zdrop = r.zdrop; j.end_bonus = r.end_bonus; j.flag = r.flag | (r.want_zd && r.step == 1 ? WM_KSW_F_ZDWALK : 0); j.step = (int8_t)r.step; j.has_n = r.has_n; memset(j.pad, 0, sizeof(j.pad));
			});
			t1 = now_ms();
			bool any_zd = false;
			for (int i = 0; i < n && !any_zd; ++i) any_zd = reqs[i]->want_zd && reqs[i]->step == 1;
			if (any_zd) {           // the z-drop scans of the gap fills come back with the alignments (ksw_zdwalk_kernel)
				zd.resize(n);
				if (wm_ksw_batch_pos_zd(c, &sc, n, jobs.data(), res.data(), pool.data(), cap, &used, zd.data())) { fail("ksw"); return; }
			} else if (wm_ksw_batch_pos(c, &sc, n, jobs.data(), res.data(), pool.data(), cap, &used)) { fail("ksw"); return; }
		} else {                // host views -> one byte slab
			std::vector<wm_ksw_job_t> jobs(n);
			size_t tot = 0;
			for (int i = 0; i < n; ++i) {
				wm::KswReq &r = *reqs[i];
				jobs[i].q_off = (uint32_t)tot; tot += (size_t)r.ql;
				jobs[i].t_off = (uint32_t)tot; tot += (size_t)r.tl;
				jobs[i].qlen = r.ql; jobs[i].tlen = r.tl;
				jobs[i].w = r.w; jobs[i].zdrop = r.zdrop; jobs[i].end_bonus = r.end_bonus; jobs[i].flag = r.flag;
			}
			if (tot >= ((size_t)1 << 32)) { error = "ksw batch exceeds 4 GB of sequence"; return; }
			UBuf<uint8_t> seqs(tot + 1, c);
			wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) { reqs[i]->copy_query(seqs.data() + jobs[i].q_off); reqs[i]->copy_target(seqs.data() + jobs[i].t_off); });
			t1 = now_ms();
			if (wm_ksw_batch(c, &sc, n, jobs.data(), seqs.data(), tot, res.data(), pool.data(), cap, &used)) { fail("ksw"); return; }
		}
		const double t2 = now_ms();
		ksw_us += c->last_ms * 1e3;
		cells += c->acc_cells;
		WM_SITE("ksw.unpack");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) {
			reqs[i]->ez = res[i];
			reqs[i]->cigar.assign(pool.begin() + res[i].cig_off, pool.begin() + res[i].cig_off + res[i].n_cigar);
			reqs[i]->has_zd = !zd.empty() && reqs[i]->want_zd && reqs[i]->step == 1;
			if (reqs[i]->has_zd) reqs[i]->zd = zd[i];
		});
		t_pack += t1 - t0; t_unpack += now_ms() - t2; t_prep += c->t_prep; t_run += c->t_run; t_fetch += c->t_fetch;
	}
	// what the four final-CIGAR front ends below put in front of their device call: one position job per request, and the requests' CIGARs end to end in pinned memory
	struct FinalOps { const uint32_t *ops; size_t n; int32_t t_pos; };
	struct FinalPack { std::vector<wm_extra_pos_t> jobs; size_t tot = 0; std::optional<UBuf<uint32_t>> cig; };
	// at(request) = its FinalOps; each(i, ops, n) runs inside the parallel copy, for a front end that has to look at every op; the buffer holds `pools` x (tot + 1) words.
	// Returns false — nothing done — unless every request is resident. A batch of 2^31 ops or more leaves `error` = too_many and no buffer.
	template <class R, class At, class Each>
	bool pack_final(std::vector<R*> &reqs, const char *too_many, const char *site, size_t pools, At at, Each each, FinalPack &P)
	{
		const int n = (int)reqs.size();
		if (!resident) return false;
		for (int i = 0; i < n; ++i) if (!reqs[i]->resident()) return false;
		P.jobs.resize(n);
		for (int i = 0; i < n; ++i) {
			const R &r = *reqs[i];
			const FinalOps o = at(r);
			wm_extra_pos_t &j = P.jobs[i];
			j.qwin_off = r.qwin_off; j.qwin_len = r.qwin_len; j.q_pos = r.q_pos; j.rid = r.rid; j.t_pos = o.t_pos; j.cig_off = (uint32_t)P.tot; j.n_cigar = (int32_t)o.n;
			P.tot += o.n;
		}
		if (P.tot >= ((size_t)1 << 31)) { error = too_many; return true; }
		P.cig.emplace(pools * (P.tot + 1), c);
		WM_SITE(site);
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) {
			const FinalOps o = at(*reqs[i]);
			if (!o.n) return;
			memcpy(P.cig->data() + P.jobs[i].cig_off, o.ops, o.n * 4);
			each(i, o.ops, o.n);
		});
		return true;
	}
	static void no_each(size_t, const uint32_t*, size_t) {}
	// call(pool, cap, &used) — and once more at the size it reported, should it report WM_ENOMEM for the pool
	template <class T, class Call> static int call_retry(std::vector<T> &pool, size_t &used, Call call)
	{
		const size_t cap = pool.size();
		int rc = call(pool.data(), cap, &used);
		if (rc == WM_ENOMEM && used > cap) { const size_t need = used; pool.resize(need); rc = call(pool.data(), need, &used); }
		return rc;
	}
	// the deferred final scans of regions (mm_update_extra's walk, src/align.c:240-286) through wm_extra_batch_pos: operands as positions in the resident reads and
	// the uploaded reference, nothing but the CIGARs is shipped. Returns false — nothing done — unless every request is resident (the caller then walks on the host).
	bool extra_batch(const wm_extra_score_t &sc, std::vector<wm::ExtraReq*> &reqs)
	{
		const int n = (int)reqs.size();
		const double t0 = now_ms();
		FinalPack P;
		if (!pack_final(reqs, "extra batch exceeds 2^31 CIGAR ops", "extra.cigars", 1, [](const wm::ExtraReq &r) { return FinalOps{ r.cigar, (size_t)r.n_cigar, r.t_pos }; }, no_each, P)) return false;
		if (!P.cig) return true;
		std::vector<wm_extra_res_t> res(n);
		if (wm_extra_batch_pos(c, &sc, n, P.jobs.data(), P.cig->data(), P.tot, res.data())) { fail("extra"); return true; }
		uint64_t cols = 0;
		for (int i = 0; i < n; ++i) {
			static_assert(sizeof(wm_extra_res_t) == sizeof(wm_extra_t), "wm_extra_res_t is wm_extra_t");
			memcpy(&reqs[i]->out, &res[i], sizeof(wm_extra_t));
			cols += (uint64_t)(res[i].blen + res[i].n_ambi);
		}
		// MM_F_EQX without its own switch: the rewriting follows the scan on the host (src/align.c:285), as in DeviceOps::extra_batch
		if (n > 0 && reqs[0]->eqx) wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) { if (reqs[i]->eqx) wm::eqx_host(*reqs[i]->eqx, reqs[i]->qp, reqs[i]->tp); });
		wm::ExtraStats &st = wm::extra_stats();
		st.on_device += (uint64_t)n; ++st.calls; st.cols += cols; st.us += (uint64_t)((now_ms() - t0) * 1e3);
		return true;
	}
	// both halves of mm_update_extra (src/align.c:240-286 with mm_fix_cigar, :91-167) through wm_fix_extra_batch_pos: the stitched CIGARs go out, the fixed ones, both shifts
	// and the scan come back. Returns false — nothing done, nothing touched — unless every request is resident and the call would not refuse an op (a zero-length op
	// of code >= 3; the aligner writes none); the caller then runs the host form. (A job over WM_EXTRA_MAX_ABS or 2^31 summed lengths is refused by the call and fails
	// the mapping call, exactly as extra_batch does: finding it beforehand would cost the measuring pass a second time.)
	bool fix_extra_batch(const wm_extra_score_t &sc, std::vector<wm::FixReq*> &reqs)
	{
		const int n = (int)reqs.size();
		const double t0 = now_ms();
		FinalPack P;
		std::atomic<int> refusable(0);
		if (!pack_final(reqs, "fix batch exceeds 2^31 CIGAR ops", "fix.cigars", 2, [](const wm::FixReq &r) { return FinalOps{ r.cigar->data(), r.cigar->size(), r.t_pos }; },
		                [&](size_t, const uint32_t *cg, size_t nc) {
			uint32_t bad = 0;
			for (size_t k = 0; k < nc; ++k) bad |= (uint32_t)(cg[k] - 3u < 13u);          // (length 0 and code >= 3: the word is 3 .. 15)
			if (bad) refusable = 1;
		}, P)) return false;
		if (!P.cig) return true;
		if (refusable.load()) return false;
		const std::vector<wm_extra_pos_t> &jobs = P.jobs;
		uint32_t *cig_out = P.cig->data() + P.tot + 1;
		std::vector<wm_extra_res_t> res(n);
		std::vector<wm_fix_res_t> fr(n);
		if (wm_fix_extra_batch_pos(c, &sc, n, jobs.data(), P.cig->data(), P.tot, cig_out, fr.data(), res.data())) { fail("fix"); return true; }
		WM_SITE("fix.unpack");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) {
			wm::FixReq &r = *reqs[i];
			if (fr[i].changed) r.cigar->assign(cig_out + jobs[i].cig_off, cig_out + jobs[i].cig_off + fr[i].n_cigar);
			r.qshift = fr[i].qshift; r.tshift = fr[i].tshift;
			memcpy(&r.out, &res[i], sizeof(wm_extra_t));
			if (r.eqx) wm::eqx_host(*r.cigar, r.qp + r.qshift, r.tp + r.tshift);       // MM_F_EQX without its own switch: on the host, behind the scan (src/align.c:285)
		});
		uint64_t cols = 0;
		for (int i = 0; i < n; ++i) cols += (uint64_t)(res[i].blen + res[i].n_ambi);
		wm::FixStats &st = wm::fix_stats();
		st.on_device += (uint64_t)n; ++st.calls; st.us += (uint64_t)((now_ms() - t0) * 1e3);
		st.cols += cols;
		return true;
	}
	// the deferred = / X rewriting (mm_update_cigar_eqx, src/align.c:169-238) through wm_eqx_batch_pos: the final CIGARs go out, the rewritten ones come back. Returns
	// false — nothing done — unless every request is resident. The first capacity is the sum of the requests' cap_hint (a safe bound once the scan has run); should the
	// call still report WM_ENOMEM for the pool, it is repeated once at the size it reported.
	bool eqx_batch(std::vector<wm::EqxReq*> &reqs)
	{
		const int n = (int)reqs.size();
		const double t0 = now_ms();
		FinalPack P;
		if (!pack_final(reqs, "eqx batch exceeds 2^31 CIGAR ops", "eqx.cigars", 1, [](const wm::EqxReq &r) { return FinalOps{ r.cigar->data(), r.cigar->size(), r.t_pos }; }, no_each, P)) return false;
		if (!P.cig) return true;
		size_t cap = 16, used = 0;
		for (int i = 0; i < n; ++i) cap += (size_t)std::max<int32_t>(reqs[i]->cap_hint, (int32_t)std::min<size_t>(reqs[i]->cigar->size(), INT32_MAX));
		std::vector<wm_eqx_res_t> res(n);
		std::vector<uint32_t> pool(cap);
		if (call_retry(pool, used, [&](uint32_t *out, size_t out_cap, size_t *out_used) { return wm_eqx_batch_pos(c, n, P.jobs.data(), P.cig->data(), P.tot, out, out_cap, out_used, res.data()); })) { fail("eqx"); return true; }
		WM_SITE("eqx.unpack");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) {
			wm::EqxReq &r = *reqs[i];
			r.cigar->assign(pool.begin() + res[i].off, pool.begin() + res[i].off + res[i].n_cigar);
			r.in_place = res[i].in_place != 0;
		});
		uint64_t cols = 0;
		for (int i = 0; i < n; ++i) for (uint32_t w : *reqs[i]->cigar) if ((w & 0xf) == 7 || (w & 0xf) == 8) cols += w >> 4;
		wm::EqxStats &st = wm::eqx_stats();
		st.on_device += (uint64_t)n; ++st.calls; st.cols += cols; st.us += (uint64_t)((now_ms() - t0) * 1e3);
		return true;
	}
	// the bodies of the cs:Z / MD:Z tags (write_cs_core / write_MD_core, src/format.c:141-218) through wm_cs_batch_pos: the final CIGARs go out, text comes back. Returns
	// false — nothing done — unless every request is resident and none would be refused (an op the reference asserts against, a bound of 2^31 bytes: the host form
	// reports those). The first capacity is 1/8 of the requests' bound; should the call report WM_ENOMEM for the pool, it is repeated once at the size it reported.
	bool cs_batch(std::vector<wm::CsReq*> &reqs)
	{
		const int n = (int)reqs.size();
		if (!resident || n == 0) return false;
		const int mode = reqs[0]->mode;
		uint64_t bound = 0;
		for (int i = 0; i < n; ++i) {
			const wm::CsReq &r = *reqs[i];
			if (!r.resident() || r.mode != mode || wm_cigar_cs_check(mode, r.cigar->data(), (int)r.cigar->size()) != -1) return false;
			const int64_t b = wm_cigar_cs_bound(r.cigar->data(), (int)r.cigar->size());
			if (b >= ((int64_t)1 << 31)) return false;
			bound += (uint64_t)b;
		}
		const double t0 = now_ms();
		FinalPack P;
		if (!pack_final(reqs, "cs batch exceeds 2^31 CIGAR ops", "cs.cigars", 1, [](const wm::CsReq &r) { return FinalOps{ r.cigar->data(), r.cigar->size(), r.rs }; }, no_each, P)) return false;
		if (!P.cig) return true;
		std::vector<wm_cs_res_t> res(n);
		size_t used = 0;
		std::vector<char> pool((size_t)(bound / 8) + 64);
		if (call_retry(pool, used, [&](char *out, size_t out_cap, size_t *out_used) { return wm_cs_batch_pos(c, mode, n, P.jobs.data(), P.cig->data(), P.tot, out, out_cap, out_used, res.data()); })) { fail("cs"); return true; }
		WM_SITE("cs.unpack");
		wm::parallel_for(c->host_threads, (size_t)n, [&](size_t i) { reqs[i]->body->assign(pool.data() + res[i].off, (size_t)res[i].len); });
		wm::CsStats &st = wm::cs_stats();
		st.on_device += (uint64_t)n; ++st.calls; st.bytes += (uint64_t)used; st.us += (uint64_t)((now_ms() - t0) * 1e3);
		return true;
	}
	// the local-score requests (ksw_ll_qinit + ksw_ll_i16, src/ksw2.h:82-83: KswReq::local) through wm_ksw_ll_batch_pos: a handful of integers per job go out, three come
	// back. Returns false — nothing done — unless the reads are resident and the call would not be refused (CallOps::ll_batch hands over eligible requests only).
	bool ll_batch(const int8_t *mat, int gapo, int gape, std::vector<wm::KswReq*> &reqs)
	{
		const int n = (int)reqs.size();
		if (!resident || n == 0 || gapo <= 0 || gape <= 0 || gapo + gape > 32767) return false;
		const double t0 = now_ms();
		std::vector<wm_ll_pos_t> jobs(n);
		std::vector<wm_ll_res_t> res(n);
		uint64_t cells = 0;
		for (int i = 0; i < n; ++i) {
			const wm::KswReq &r = *reqs[i];
			wm_ll_pos_t &j = jobs[i];
			memset(&j, 0, sizeof(j));
			j.qwin_off = r.qwin_off; j.qwin_len = r.qwin_len; j.q_pos = r.q_pos; j.rid = r.rid; j.t_pos = r.t_pos; j.qlen = r.ql; j.tlen = r.tl; j.step = (int8_t)r.step;
			cells += (uint64_t)r.ql * (uint64_t)r.tl;
		}
		if (wm_ksw_ll_batch_pos(c, mat, gapo, gape, n, jobs.data(), res.data())) { fail("ksw_ll"); return true; }
		for (int i = 0; i < n; ++i) { reqs[i]->ez.max = res[i].score; reqs[i]->ez.max_q = res[i].qe; reqs[i]->ez.max_t = res[i].te; }
		wm::LlStats &st = wm::ll_stats();
		st.on_device += (uint64_t)n; ++st.calls; st.cells += cells; st.us += (uint64_t)((now_ms() - t0) * 1e3);
		return true;
	}
	// splice mode (src/align.c:326-327): the requests through wm_ksw_exts2_batch, in groups whose unbanded traceback matrices fit the arena
	void exts2_batch(const wm_ksw_score_t &sc, int noncan, int junc_bonus, std::vector<wm::KswReq*> &reqs)
	{
		const size_t budget = (size_t)(c->arena_bytes * 0.6);
		const int n = (int)reqs.size();
		if (n > 0) ++g_exts2_calls;
		for (int i0 = 0; i0 < n;) {
			size_t need = 0, tot = 0, cap = 16;
			int i1 = i0;
			for (; i1 < n; ++i1) {
				const wm::KswReq &r = *reqs[i1];
				const size_t n_col = (size_t)((((r.ql < r.tl ? r.ql : r.tl) + 15) / 16 + 1) * 16);
				const size_t b = ((size_t)r.ql + r.tl) * (n_col + 10) + 16 * (size_t)r.tl + 1024;      // traceback + CIGAR slots + operands + row state
				if (i1 > i0 && (need + b > budget || tot + r.ql + r.tl >= ((size_t)1 << 31))) break;
				need += b; tot += (size_t)r.ql + r.tl; cap += (size_t)r.ql + r.tl + 2;
			}
			const int m = i1 - i0;
			++g_exts2_groups;
			std::vector<wm_ksw_job_t> jobs(m);
			std::vector<wm_ksw_result_t> res(m);
			std::vector<uint8_t> seqs(tot + 1), junc;
			std::vector<uint32_t> pool(cap);
			size_t off = 0, used = 0;
			bool any_junc = false;
			for (int i = 0; i < m; ++i) any_junc |= !reqs[i0 + i]->junc.empty();
			if (any_junc) junc.assign(tot + 1, 0);                     // parallel to seqs: junction bits at the targets (mm_idx_bed_junc, src/index.c:768-803)
			for (int i = 0; i < m; ++i) {
				wm::KswReq &r = *reqs[i0 + i];
				jobs[i].q_off = (uint32_t)off; off += (size_t)r.ql;
				jobs[i].t_off = (uint32_t)off; off += (size_t)r.tl;
				jobs[i].qlen = r.ql; jobs[i].tlen = r.tl; jobs[i].w = -1; jobs[i].zdrop = r.zdrop; jobs[i].end_bonus = 0; jobs[i].flag = r.flag;
			}
			wm::parallel_for(c->host_threads, (size_t)m, [&](size_t i) {
				const wm::KswReq &r = *reqs[i0 + i];
				r.copy_query(seqs.data() + jobs[i].q_off); r.copy_target(seqs.data() + jobs[i].t_off);
				if (!r.junc.empty()) memcpy(junc.data() + jobs[i].t_off, r.junc.data(), r.junc.size());
			});
			if (wm_ksw_exts2_batch(c, &sc, noncan, junc_bonus, m, jobs.data(), seqs.data(), tot, any_junc ? junc.data() : 0, res.data(), pool.data(), cap, &used)) { fail("ksw_exts2"); return; }
			for (int i = 0; i < m; ++i) {
				reqs[i0 + i]->ez = res[i];
				reqs[i0 + i]->cigar.assign(pool.begin() + res[i].cig_off, pool.begin() + res[i].cig_off + res[i].n_cigar);
			}
			i0 = i1;
		}
	}
};

// The product's DeviceOps: a pool of device contexts. Every batched call borrows a free context (its own HIP stream, arena and pinned
// slab), so up to max_inflight() batches — of the same or of different operations — are on the device at once, issued by different
// host threads (wm_fiber.h).
struct GpuOps {                          // the device contexts of a mapper, shared by its (at most WM_MAX_SLOTS concurrent) mapping calls: see CallOps
	std::vector<GpuOpsCtx> ctxs;
	std::vector<int> free_;
	std::mutex mu;
	std::condition_variable cv;
	void init(const std::vector<wm_ctx_t*> &cs) { ctxs.resize(cs.size()); for (size_t i = 0; i < cs.size(); ++i) { ctxs[i].c = cs[i]; free_.push_back((int)i); } }
	int max_inflight() const { return (int)ctxs.size(); }
	bool waits_asleep() const { return getenv("WM_SPIN_SYNC") == 0; }
	// The read codes of a mini-batch go to the device once. Up to WM_MAX_SLOTS mini-batches can be in flight (concurrent mapping calls, one slot each): one
	// allocation of WM_MAX_SLOTS slabs, owned by the first context and aliased by the others (one device); a call's offsets start at slot * slab.
	std::mutex reads_mu;
	hipStream_t up_stream = 0;                  // uploads of the mini-batches' read codes
	uint64_t *stage[WM_MAX_SLOTS] = { 0 }; size_t stage_words[WM_MAX_SLOTS] = { 0 }; bool stage_pinned[WM_MAX_SLOTS] = { false };      // host staging of the packed codes, per slot
	~GpuOps()
	{
		if (up_stream) hipStreamDestroy(up_stream);
		for (int i = 0; i < WM_MAX_SLOTS; ++i) if (stage[i]) { if (stage_pinned[i]) hipHostFree(stage[i]); else free(stage[i]); }
	}
	size_t slab = 0;
	int n_slabs = 0;
	std::atomic<int> slots_hint{0};             // mini-batches the caller keeps in flight: wm_mapper_set_slots, the lanes of wm_map_file[_multi], or the highest slot seen + 1
	bool slot_busy[WM_MAX_SLOTS] = { false };
	bool load_reads(const uint8_t *codes, size_t n, int slot, int64_t *base, std::string &err)
	{
		*base = 0;
		const bool off = getenv("WM_NO_RESIDENT") != 0;            // A/B switch: per-request staging as before
		if (off || ctxs.empty() || slot < 0 || slot >= WM_MAX_SLOTS) return false;
		wm_ctx_t *c0 = ctxs[0].c;
		std::lock_guard<std::mutex> lk(reads_mu);
		if (hipSetDevice(c0->device) != hipSuccess) return false;
		if (slot + 1 > slots_hint.load()) slots_hint = slot + 1;
		if (n + 256 > slab || slot >= n_slabs || !c0->d_reads || !c0->owns_reads) {
			for (int o = 0; o < WM_MAX_SLOTS; ++o) if (o != slot && slot_busy[o]) {      // another mini-batch lives in the allocation: this one is served from its host views
				static std::atomic<bool> told(false);
				if (!told.exchange(true)) fprintf(stderr, "[wmgpu] mini-batch on slot %d is served from host views (no resident slab: %d slab(s) of %zu bases, another slot busy); "
				                                  "tell the mapper how many mini-batches are in flight (wm_mapper_set_slots / WM_READ_SLABS)\n", slot, n_slabs, slab);
				return false;
			}
			if (c0->d_reads && c0->owns_reads) hipFree(c0->d_reads);
			c0->d_reads = 0; c0->owns_reads = false; slab = 0;
			const size_t want = (n + n / 8 + (1 << 20) + 255) & ~(size_t)255;
			// slabs for the mini-batches that can be in flight: WM_READ_SLABS, else the lanes of wm_map_file (WM_MAP_LANES), at least 2 (four were
			// allocated whatever the caller used — 4.5 GB for 1-Gbase mini-batches); a call on a slot beyond them is served from its host views
			n_slabs = std::max(2, std::min((int)WM_MAX_SLOTS, getenv("WM_READ_SLABS") ? atoi(getenv("WM_READ_SLABS")) : std::max(slots_hint.load(), getenv("WM_MAP_LANES") ? atoi(getenv("WM_MAP_LANES")) : 2)));
			if (slot >= n_slabs) n_slabs = slot + 1;
			if (reads_alloc(c0, (size_t)n_slabs * want) != WM_OK) return false;              // (bases: 2 bits + 1 ambiguity bit each, reads2bit.h)
			c0->owns_reads = true; c0->reads_bytes = (size_t)n_slabs * want; slab = want;
			for (size_t i = 1; i < ctxs.size(); ++i) {
				wm_ctx_t *c = ctxs[i].c;
				if (c->owns_reads && c->d_reads) hipFree(c->d_reads);
				c->d_reads = c0->d_reads; c->d_reads_nm = c0->d_reads_nm; c->reads_bytes = c0->reads_bytes; c->reads_cap = 0; c->owns_reads = false;
			}
		}
		// the mini-batch's codes are packed on the host — 2 bits per base + 1 ambiguity bit, 0.375 B per base across PCIe instead of one byte — into this slot's
		// pinned staging buffer, by a few threads over disjoint 64-base-aligned ranges (slab is a multiple of 256 bases: the slot's words are its own)
		const size_t pkw = wm_pk_words(n), nmw = wm_nm_words(n);
		if (stage_words[slot] < pkw + nmw) {
			if (stage[slot]) { if (stage_pinned[slot]) hipHostFree(stage[slot]); else free(stage[slot]); }
			stage[slot] = 0; stage_words[slot] = 0;
			const size_t want_w = pkw + nmw + (pkw + nmw) / 8 + 1024;
			stage_pinned[slot] = hipHostMalloc((void**)&stage[slot], want_w * 8, hipHostMallocDefault) == hipSuccess;
			if (!stage_pinned[slot]) { (void)hipGetLastError(); stage[slot] = (uint64_t*)malloc(want_w * 8); }
			if (!stage[slot]) { err = "no host memory for the packed reads"; return false; }
			stage_words[slot] = want_w;
		}
		uint64_t *h_pk = stage[slot], *h_nm = stage[slot] + pkw;
		{
			const size_t CH = (size_t)1 << 22;                     // bases per range (a multiple of 64)
			const size_t n_ch = (n + CH - 1) / CH;
			const int nt = (int)std::max<size_t>(1, std::min<size_t>(std::min<size_t>(8, (size_t)wm::usable_cores()), n_ch));
			wm::parallel_for(nt, n_ch, [&](size_t ci) { const size_t at = ci * CH, len = std::min(CH, n - at); wm_pack_blocks(codes + at, len, h_pk + at / 32, h_nm + at / 64); });
			for (size_t i = 2 * ((n + 63) / 64); i < pkw; ++i) h_pk[i] = 0;
			for (size_t i = (n + 63) / 64; i < nmw; ++i) h_nm[i] = 0;
		}
		// (a stream of its own, not the NULL stream: a NULL-stream copy waits for every blocking stream of the device and makes them wait for it)
		if (!up_stream && hipStreamCreateWithFlags(&up_stream, hipStreamNonBlocking) != hipSuccess) { up_stream = 0; (void)hipGetLastError(); }
		uint64_t *d_pk = c0->d_reads + (size_t)slot * slab / 32, *d_nm = c0->d_reads_nm + (size_t)slot * slab / 64;
		if (n && (up_stream ? (hipMemcpyAsync(d_pk, h_pk, pkw * 8, hipMemcpyHostToDevice, up_stream) != hipSuccess || hipMemcpyAsync(d_nm, h_nm, nmw * 8, hipMemcpyHostToDevice, up_stream) != hipSuccess ||
		                       hipStreamSynchronize(up_stream) != hipSuccess)
		                    : (hipMemcpy(d_pk, h_pk, pkw * 8, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(d_nm, h_nm, nmw * 8, hipMemcpyHostToDevice) != hipSuccess))) {
			err = std::string("reads upload: ") + hipGetErrorString(hipGetLastError()); return false;
		}
		for (GpuOpsCtx &x : ctxs) x.resident = true;
		slot_busy[slot] = true;
		*base = (int64_t)((size_t)slot * slab);
		return true;
	}
	void release_reads(int slot) { std::lock_guard<std::mutex> lk(reads_mu); if (slot >= 0 && slot < WM_MAX_SLOTS) slot_busy[slot] = false; }
	// One batched call on a free context. A context belongs to exactly one call while it is out of the free list, so whatever the call leaves in
	// the context's `error` is ITS error: it moves into the sink of the mapping call that issued the batch before the context is handed back
	// (two mapping calls share the contexts, wm_map_reads_slot). A mapping call that has failed issues nothing more.
	template <class F> void with(wm::ErrorSink &sink, F f)
	{
		{ std::lock_guard<std::mutex> lk(sink.mu); if (!sink.msg.empty()) return; }
		int i;
		{ std::unique_lock<std::mutex> lk(mu); cv.wait(lk, [&] { return !free_.empty(); }); i = free_.back(); free_.pop_back(); }
		ctxs[i].error.clear();
		try { f(ctxs[i]); }
		catch (const std::exception &e) { if (ctxs[i].error.empty()) ctxs[i].error = std::string("batched device call: ") + e.what(); }
		if (!ctxs[i].error.empty()) { sink.put(ctxs[i].error); ctxs[i].error.clear(); }
		{ std::lock_guard<std::mutex> lk(mu); free_.push_back(i); }
		cv.notify_one();
	}
	// a batch whose buffers do not fit the context's arena is served in halves (recursively): the hub sizes batches by demand, not by HBM
	template <class R, class F> static void run_split(GpuOpsCtx &x, std::vector<R*> &reqs, F f)
	{
		if (!x.error.empty()) return;          // an earlier part of this call failed for good: nothing more is attempted (and nothing is cleared)
		f(reqs);
		if (x.error.empty() || reqs.size() < 2 || x.error.find("does not fit the arena") == std::string::npos) { ++g_split_parts; return; }
		x.error.clear();                       // (set by THIS call: the context was clean on entry)
		++g_split_halved;
		std::vector<R*> a(reqs.begin(), reqs.begin() + reqs.size() / 2), b(reqs.begin() + reqs.size() / 2, reqs.end());
		run_split(x, a, f);
		if (x.error.empty()) run_split(x, b, f);
	}
	void sketch_batch(wm::ErrorSink &e, int w, int k, std::vector<wm::SketchReq*> &reqs) { with(e, [&](GpuOpsCtx &x) { run_split(x, reqs, [&](std::vector<wm::SketchReq*> &part) { x.sketch_batch(w, k, part); }); }); }
	void seed_batch(wm::ErrorSink &e, std::vector<wm::SeedReq*> &reqs) { with(e, [&](GpuOpsCtx &x) { run_split(x, reqs, [&](std::vector<wm::SeedReq*> &part) { x.seed_batch(part); }); }); }
	void chain_batch(wm::ErrorSink &e, std::vector<wm::ChainReq*> &reqs) { with(e, [&](GpuOpsCtx &x) { run_split(x, reqs, [&](std::vector<wm::ChainReq*> &part) { x.chain_batch(part); }); }); }
	void ksw_batch(wm::ErrorSink &e, const wm_ksw_score_t &sc, std::vector<wm::KswReq*> &reqs) { with(e, [&](GpuOpsCtx &x) { x.ksw_batch(sc, reqs); }); }
	void exts2_batch(wm::ErrorSink &e, const wm_ksw_score_t &sc, int noncan, int junc_bonus, std::vector<wm::KswReq*> &reqs) { with(e, [&](GpuOpsCtx &x) { x.exts2_batch(sc, noncan, junc_bonus, reqs); }); }
	// *served = false: some request is not resident (or the mapping call has failed already): nothing was done
	void extra_batch(wm::ErrorSink &e, const wm_extra_score_t &sc, std::vector<wm::ExtraReq*> &reqs, bool *served)
	{
		*served = false;
		with(e, [&](GpuOpsCtx &x) { bool all = true; run_split(x, reqs, [&](std::vector<wm::ExtraReq*> &part) { all = x.extra_batch(sc, part) && all; }); *served = all; });
	}
	// the final-pass calls that may decline a part: call(x, part) = false leaves the part untouched, and it goes to `rest` (not resident, or refusable) — as does
	// everything when the mapping call has failed already and nothing was issued
	template <class R, class F> void batch_or_rest(wm::ErrorSink &e, std::vector<R*> &reqs, std::vector<R*> &rest, F call)
	{
		bool ran = false;
		with(e, [&](GpuOpsCtx &x) { ran = true; run_split(x, reqs, [&](std::vector<R*> &part) { if (!call(x, part)) rest.insert(rest.end(), part.begin(), part.end()); }); });
		if (!ran) rest = reqs;
	}
	// collect_seed_hits takes one (max_occ, flag) per call: the mapper's requests of one mapping call all share them
	void window_batch(wm::ErrorSink &e, std::vector<wm::WindowReq*> &reqs) { with(e, [&](GpuOpsCtx &x) { run_split(x, reqs, [&](std::vector<wm::WindowReq*> &part) { x.window_batch(part); }); }); }
};

// What ONE mapping call hands to wm::map_batch: the shared contexts behind it, and the call's own error sink — the first failed batch of this
// call fails this call and no other (a per-context error field let the call that finished first take, and clear, its neighbour's).
struct CallOps : wm::DeviceOps {
	GpuOps &g;
	wm::ErrorSink err;
	explicit CallOps(GpuOps &g_) : g(g_) {}
	int max_inflight() const override { return g.max_inflight(); }
	bool waits_asleep() const override { return g.waits_asleep(); }
	bool load_reads(const uint8_t *codes, size_t n, int slot, int64_t *base) override
	{
		std::string e;
		const bool ok = g.load_reads(codes, n, slot, base, e);
		if (!e.empty()) err.put(e);
		return ok;
	}
	void release_reads(int slot) override { g.release_reads(slot); }
	void sketch_batch(int w, int k, std::vector<wm::SketchReq*> &reqs) override { g.sketch_batch(err, w, k, reqs); }
	void seed_batch(std::vector<wm::SeedReq*> &reqs) override { g.seed_batch(err, reqs); }
	void chain_batch(std::vector<wm::ChainReq*> &reqs) override { g.chain_batch(err, reqs); }
	void ksw_batch(const wm_ksw_score_t &sc, std::vector<wm::KswReq*> &reqs) override { g.ksw_batch(err, sc, reqs); }
	void exts2_batch(const wm_ksw_score_t &sc, int noncan, int junc_bonus, std::vector<wm::KswReq*> &reqs) override { g.exts2_batch(err, sc, noncan, junc_bonus, reqs); }
	void window_batch(int, int, std::vector<wm::WindowReq*> &reqs) override { g.window_batch(err, reqs); }
	void extra_batch(const wm_extra_score_t &sc, std::vector<wm::ExtraReq*> &reqs) override
	{
		bool served = false;
		g.extra_batch(err, sc, reqs, &served);
		if (!served) wm::DeviceOps::extra_batch(sc, reqs);          // a request that is not resident: the host walk (counted by wm_extra_stats)
	}
	void fix_extra_batch(const wm_extra_score_t &sc, std::vector<wm::FixReq*> &reqs) override
	{
		std::vector<wm::FixReq*> rest;
		g.batch_or_rest(err, reqs, rest, [&](GpuOpsCtx &x, std::vector<wm::FixReq*> &part) { return x.fix_extra_batch(sc, part); });
		if (!rest.empty()) wm::DeviceOps::fix_extra_batch(sc, rest);       // not resident: the host specification + walk (counted by wm_fix_stats)
	}
	void cs_batch(std::vector<wm::CsReq*> &reqs) override
	{
		std::vector<wm::CsReq*> rest;
		g.batch_or_rest(err, reqs, rest, [](GpuOpsCtx &x, std::vector<wm::CsReq*> &part) { return x.cs_batch(part); });
		if (!rest.empty()) wm::DeviceOps::cs_batch(rest);                  // not resident, or the device call would refuse it: the host specification (counted by wm_cs_stats)
	}
	void ll_batch(const int8_t *mat, int gapo, int gape, std::vector<wm::KswReq*> &reqs) override
	{
		std::vector<wm::KswReq*> dev, rest;
		for (wm::KswReq *r : reqs) (r->resident() && r->ql >= 1 && r->tl >= 1 && r->ql <= WM_LL_MAX_LEN && r->tl <= WM_LL_MAX_LEN ? dev : rest).push_back(r);
		if (!dev.empty()) g.batch_or_rest(err, dev, rest, [&](GpuOpsCtx &x, std::vector<wm::KswReq*> &part) { return x.ll_batch(mat, gapo, gape, part); });
		if (!rest.empty()) wm::DeviceOps::ll_batch(mat, gapo, gape, rest);    // not resident, or longer than WM_LL_MAX_LEN: the host form (counted by wm_ll_stats)
	}
	void eqx_batch(std::vector<wm::EqxReq*> &reqs) override
	{
		std::vector<wm::EqxReq*> rest;
		g.batch_or_rest(err, reqs, rest, [](GpuOpsCtx &x, std::vector<wm::EqxReq*> &part) { return x.eqx_batch(part); });
		if (!rest.empty()) wm::DeviceOps::eqx_batch(rest);                 // not resident: the host specification (counted by wm_eqx_stats)
	}
};

struct wm_mapper_s {
	wm_ctx_t *c; const wm_index_t *idx;
	std::vector<wm_ctx_t*> workers;        // extra contexts (own stream + arena slice) for groups 1..G-1
	int n_threads = 1;
	int n_threads_cap = 0;                 // > 0: a file loop over several mappers has divided the host's cores among its mapping calls (wm_map_file_multi)
	int call_threads() const { return n_threads_cap > 0 && n_threads_cap < n_threads ? n_threads_cap : n_threads; }
	wm::IdxOpt io; wm::MapOpt mo;
	// results of the last mapping call per slot (wm_map_reads = slot 0; wm_map_reads_slot: two calls may run concurrently)
	struct Result { std::string text; std::vector<int32_t> hits; std::vector<uint32_t> cigars; std::vector<int64_t> first; std::vector<uint8_t> rl_defined; } res[WM_MAX_SLOTS];
	uint64_t stats[9];
	double host_stats[24] = {0};
	std::mutex stats_mu;
	std::unique_ptr<GpuOps> ops;           // the device contexts as a pool shared by the mapping calls (created on first use, rebuilt by wm_mapper_set_threads)
	int slots_hint = 0;                    // wm_mapper_set_slots
	bool sam_header = true;                // wm_map_file writes the @SQ / @PG lines (wm_mapper_set_sam_header)
	std::vector<std::string> cmdline;      // argv of the front end, for the @PG line of SAM files (wm_mapper_set_cmdline)
};

// what the mapper's device path does not serve is refused when the mapper is made, not in the middle of a mapping call. An even k: the
// fused window call sketches it (sketch_kernel.h: sketch_even_steps, the palindrome rule of src/sketch.c:166), but the mapper serves it only to a process
// that has opted in — wm_set_even_k(1), or WM_EVEN_K=1 in the environment, which is read whenever a mapper is made. An index built with homopolymer
// compression (MM_I_HPC, -H) is served since round 5: sketch_coop compacts every sequence into its runs first (src/sketch.c:152-163), mm_adjust_minier's
// HPC branch (src/align.c:352-361) runs on the host.
static std::atomic<int> g_even_k(-1);          // -1: the environment decides
static bool even_k_on()
{
	const int v = g_even_k.load(std::memory_order_relaxed);
	if (v >= 0) return v != 0;
	const char *e = getenv("WM_EVEN_K");
	return e && atoi(e) != 0;
}
extern "C" void wm_set_even_k(int on) { g_even_k = on < 0 ? -1 : on ? 1 : 0; }
extern "C" int wm_even_k_enabled(void) { return even_k_on(); }
static int mapper_index_ok(const wm_index_t *idx)
{
	if (!(idx->ix.k & 1) && !even_k_on())
		return set_err(WM_EINVAL, "k = %d: the mapper's device path needs an odd k (every preset of the reference has one) unless even k is switched on: wm_set_even_k(1) or WM_EVEN_K=1", idx->ix.k);
	return WM_OK;
}
extern "C" int wm_mapper_create(wm_ctx_t *c, const wm_index_t *idx, const char *preset, int64_t flag, wm_mapper_t **out)
{
	*out = 0;
	if (!c || !idx) return set_err(WM_EINVAL, "null argument");
	if (!c->have_index) return set_err(WM_EINVAL, "wm_index_upload has not been called on this context");
	if (mapper_index_ok(idx)) return WM_EINVAL;
	wm_default_malloc();
	wm_mapper_t *m = new wm_mapper_t();
	m->c = c; m->idx = idx;
	wm::set_preset(0, m->io, m->mo);
	if (preset && preset[0] && wm::set_preset(preset, m->io, m->mo) < 0) { delete m; return set_err(WM_EINVAL, "unknown preset '%s'", preset); }
	m->mo.flag |= flag;
	m->io.k = idx->ix.k; m->io.w = idx->ix.w;
	wm::mapopt_update(m->mo, idx->ix);
	std::string err;
	if (wm::check_opt(m->io, m->mo, err) < 0) { delete m; return set_err(WM_EINVAL, "%s", err.c_str()); }
	memset(m->stats, 0, sizeof(m->stats));
	*out = m;
	return WM_OK;
}
#define WM_MAPOPT_FIELDS(X) X(flag) X(seed) X(sdust_thres) X(max_qlen) X(bw) X(max_gap) X(max_gap_ref) X(min_gap_ref) X(max_frag_len) \
	X(max_chain_skip) X(max_chain_iter) X(min_cnt) X(min_chain_score) X(chain_gap_scale) X(SVawareMinReadLength) X(suffixSampleOffset) X(min_mapq) \
	X(min_qcov) X(minPrefixLength) X(maxPrefixLength) X(prefixIncrementFactor) X(stage2_bw) X(stage2_zdrop_inv) X(stage2_max_gap) X(mask_level) \
	X(mask_len) X(pri_ratio) X(best_n) X(max_join_long) X(max_join_short) X(min_join_flank_sc) X(min_join_flank_ratio) X(alt_drop) X(a) X(b) X(q) X(e) \
	X(q2) X(e2) X(sc_ambi) X(zdrop) X(zdrop_inv) X(end_bonus) X(min_dp_max) X(min_ksw_len) X(max_clip_ratio) X(mid_occ_frac) X(min_mid_occ) X(mid_occ) \
	X(max_occ) X(mini_batch_size) X(max_sw_mat) X(noncan) X(junc_bonus) X(anchor_ext_len) X(anchor_ext_shift)
static void mapopt_to_c(const wm::MapOpt &o, wm_mapopt_t *c)
{
	memset(c, 0, sizeof(*c));
#define X(f) c->f = (decltype(c->f))o.f;
	WM_MAPOPT_FIELDS(X)
#undef X
	c->SVaware = o.SVaware ? 1 : 0;
}
static void mapopt_from_c(const wm_mapopt_t *c, wm::MapOpt &o)
{
#define X(f) o.f = (decltype(o.f))c->f;
	WM_MAPOPT_FIELDS(X)
#undef X
	o.SVaware = c->SVaware != 0;
}
extern "C" int wm_mapopt_preset(const char *preset, wm_mapopt_t *out, int *k, int *w)
{
	wm::IdxOpt io; wm::MapOpt mo;
	wm::set_preset(0, io, mo);
	if (preset && preset[0] && wm::set_preset(preset, io, mo) < 0) return set_err(WM_EINVAL, "unknown preset '%s'", preset);
	mapopt_to_c(mo, out);
	if (k) *k = io.k;
	if (w) *w = io.w;
	return WM_OK;
}
extern "C" int wm_mapper_create_opt(wm_ctx_t *c, const wm_index_t *idx, const wm_mapopt_t *opt, wm_mapper_t **out)
{
	*out = 0;
	if (!c || !idx || !opt) return set_err(WM_EINVAL, "null argument");
	if (!c->have_index) return set_err(WM_EINVAL, "wm_index_upload has not been called on this context");
	if (mapper_index_ok(idx)) return WM_EINVAL;
	wm_default_malloc();
	wm_mapper_t *m = new wm_mapper_t();
	m->c = c; m->idx = idx;
	wm::set_preset(0, m->io, m->mo);
	mapopt_from_c(opt, m->mo);
	m->io.k = idx->ix.k; m->io.w = idx->ix.w;
	wm::mapopt_update(m->mo, idx->ix);
	std::string err;
	if (wm::check_opt(m->io, m->mo, err) < 0) { delete m; return set_err(WM_EINVAL, "%s", err.c_str()); }
	memset(m->stats, 0, sizeof(m->stats));
	*out = m;
	return WM_OK;
}
extern "C" int wm_mapper_set_sam_header(wm_mapper_t *m, int on) { if (!m) return set_err(WM_EINVAL, "null mapper"); m->sam_header = on != 0; return WM_OK; }

extern "C" void wm_mapper_destroy(wm_mapper_t *m)
{
	if (!m) return;
	if (wm::prof_on()) wm::prof_report(stderr);                // WM_PROF=1: the host glue's time per named region (accumulated over the process)
	for (wm_ctx_t *w : m->workers) wm_ctx_destroy(w);
	delete m;
}

// Host parallelism: n_threads worker threads run the host glue of the reads (fibers, wm_fiber.h) and take turns issuing the batched
// device calls; C device contexts (own HIP stream + arena + pinned slab each; WM_CONTEXTS, default 4) let C batches be in flight at once.
extern "C" int wm_mapper_set_threads(wm_mapper_t *m, int n_threads, size_t arena_bytes_per_context)
{
	if (n_threads < 1) return set_err(WM_EINVAL, "n_threads < 1");
	for (wm_ctx_t *w : m->workers) wm_ctx_destroy(w);
	m->workers.clear();
	m->ops.reset();
	int C = getenv("WM_CONTEXTS") ? atoi(getenv("WM_CONTEXTS")) : (getenv("WM_GROUPS") ? atoi(getenv("WM_GROUPS")) : (n_threads >= 8 ? 6 : n_threads >= 2 ? 2 : 1));
	if (C < 1) C = 1;
	m->n_threads = n_threads;
	const int bt = getenv("WM_BATCH_THREADS") ? atoi(getenv("WM_BATCH_THREADS")) : 1;     // extra threads a batched call may spawn for its own packing
	m->c->host_threads = std::max(1, bt);
	for (int g = 1; g < C; ++g) {
		wm_ctx_t *w = 0;
		const int rc = wm_ctx_create(m->c->device, arena_bytes_per_context ? arena_bytes_per_context : m->c->arena_bytes, &w);
		if (rc) return rc;
		w->d_hkey = m->c->d_hkey; w->d_hval = m->c->d_hval; w->d_P = m->c->d_P; w->d_bloom = m->c->d_bloom; w->hbits = m->c->hbits; w->skp = m->c->skp;
		w->d_S = m->c->d_S; w->d_name_rank = m->c->d_name_rank; w->d_seq_len = m->c->d_seq_len; w->seq_off = m->c->seq_off; w->seq_len = m->c->seq_len;
		w->have_index = true; w->owns_index = false;
		w->host_threads = m->c->host_threads;
		m->workers.push_back(w);
	}
	// side streams: one pool for all contexts, so that main streams + pool = the hardware queues (WM_SIDE_POOL overrides the pool size)
	{
		const int hwq = getenv("GPU_MAX_HW_QUEUES") ? atoi(getenv("GPU_MAX_HW_QUEUES")) : 4;
		int P = getenv("WM_SIDE_POOL") ? atoi(getenv("WM_SIDE_POOL")) : std::max(0, hwq - C);
		if (C == 1) P = 0;                                   // a single context keeps its own side streams
		wm_ctx_t *c0 = m->c;                                  // (the pool lives and dies with the mapper's first context)
		HIPCHK(hipStreamSynchronize(c0->stream));
		// (compute units of their own for the heavy / huge calls' side streams — hipExtStreamCreateWithCUMask, VERDICT r4 item 2 iii — were measured in round 5:
		// 0.075 / 0.118 / 0.174 Gbp/s with 32 / 64 / 96 CUs against 0.257 without; profiles/r05_sched.txt. The few hundred latency-bound wavefronts of a
		// stripe launch need the whole chip's SIMDs.)
		while ((int)c0->owned_pool.size() > P) { hipStreamDestroy(c0->owned_pool.back()); c0->owned_pool.pop_back(); }
		while ((int)c0->owned_pool.size() < P) { hipStream_t st; HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking)); c0->owned_pool.push_back(st); }
		c0->side_pool = P > 0 ? c0->owned_pool.data() : 0; c0->n_side_pool = P; c0->side_next = c0->owned_next;
		for (wm_ctx_t *w : m->workers) { w->side_pool = c0->side_pool; w->n_side_pool = P; w->side_next = c0->owned_next; }
	}
	// the pinned staging slabs are allocated now, not inside the first mapping call (page-locking a few GB takes a noticeable fraction of a second)
	{ size_t mark = 0; if (pin_take(m->c, 1, &mark)) pin_release(m->c, mark); }
	for (wm_ctx_t *w : m->workers) { size_t mark = 0; if (pin_take(w, 1, &mark)) pin_release(w, mark); }
	return WM_OK;
}

static int map_reads_impl(wm_mapper_t *m, std::vector<wm::ReadIn> &reads, double tm0, int slot = 0);

extern "C" int wm_map_reads(wm_mapper_t *m, int n, const char *const *names, const char *const *seqs, const int32_t *lens,
                            const char **text, size_t *text_len, const int32_t **hits, const uint32_t **cigars, const int64_t **hit_first)
{
	const double tm0 = now_ms();
	std::vector<wm::ReadIn> reads(n);
	wm::parallel_for(m->n_threads, (size_t)n, [&](size_t i) { reads[i].name = names[i]; reads[i].seq.assign(seqs[i], lens[i]); });
	const int rc = map_reads_impl(m, reads, tm0, 0);
	if (rc) return rc;
	if (text) *text = m->res[0].text.data();
	if (text_len) *text_len = m->res[0].text.size();
	if (hits) *hits = m->res[0].hits.data();
	if (cigars) *cigars = m->res[0].cigars.data();
	if (hit_first) *hit_first = m->res[0].first.data();
	return WM_OK;
}

// wm_map_reads with its own result buffers and its own slab of resident read codes: calls with different slots (0 and 1) may run concurrently from two
// host threads. A mapping call spends its first and last few hundred milliseconds filling and draining its pipeline of dependent device calls (window
// -> align -> align -> window -> align ...): with two mini-batches in flight those phases of one hide behind the steady state of the other.
extern "C" int wm_map_reads_slot(wm_mapper_t *m, int slot, int n, const char *const *names, const char *const *seqs, const int32_t *lens,
                                 const char **text, size_t *text_len, const int32_t **hits, const uint32_t **cigars, const int64_t **hit_first)
{
	if (!m || slot < 0 || slot >= WM_MAX_SLOTS) return set_err(WM_EINVAL, "slot must be 0 .. WM_MAX_SLOTS - 1");
	const double tm0 = now_ms();
	std::vector<wm::ReadIn> reads(n);
	wm::parallel_for(m->n_threads, (size_t)n, [&](size_t i) { reads[i].name = names[i]; reads[i].seq.assign(seqs[i], lens[i]); });
	const int rc = map_reads_impl(m, reads, tm0, slot);
	if (rc) return rc;
	wm_mapper_t::Result &R = m->res[slot];
	if (text) *text = R.text.data();
	if (text_len) *text_len = R.text.size();
	if (hits) *hits = R.hits.data();
	if (cigars) *cigars = R.cigars.data();
	if (hit_first) *hit_first = R.first.data();
	return WM_OK;
}

// the device contexts of a mapper as the pool its mapping calls share (caller holds m->stats_mu)
static void ensure_ops(wm_mapper_t *m)
{
	if (m->ops) return;
	m->ops.reset(new GpuOps());
	std::vector<wm_ctx_t*> cs; cs.push_back(m->c); cs.insert(cs.end(), m->workers.begin(), m->workers.end());
	m->ops->init(cs);
	m->ops->slots_hint = m->slots_hint;
}

// how many mini-batches the caller keeps in flight on this mapper (wm_map_reads_slot on slots 0 .. n - 1): the resident-reads allocation gets that many slabs
// the next time it is (re)made (a caller of slots 2..3 was silently served from host views)
extern "C" int wm_mapper_set_slots(wm_mapper_t *m, int n)
{
	if (!m || n < 1 || n > WM_MAX_SLOTS) return set_err(WM_EINVAL, "slots must be 1 .. WM_MAX_SLOTS");
	std::lock_guard<std::mutex> lk(m->stats_mu);
	if (n > m->slots_hint) m->slots_hint = n;
	ensure_ops(m);
	if (n > m->ops->slots_hint.load()) m->ops->slots_hint = n;
	return WM_OK;
}

// per read of the slot's last mapping call: 1 = the mapper assigned rep_len where the reference assigns it (src/map.c:808-813 rescan, :859-861 fallback),
// 0 = the pure-MCAS path, where the reference feeds mm_set_mapq an uninitialised word (src/map.c:281,933) and MAPQ / rl:i are not comparable
extern "C" int wm_map_reads_rep_len_defined(const wm_mapper_t *m, int slot, const uint8_t **flags, size_t *n)
{
	if (!m || slot < 0 || slot >= WM_MAX_SLOTS || !flags) return set_err(WM_EINVAL, "bad argument");
	*flags = m->res[slot].rl_defined.data();
	if (n) *n = m->res[slot].rl_defined.size();
	return WM_OK;
}

// maps `reads` in the given order; results land in m->text / hits / cigars / first / stats
static int map_reads_impl(wm_mapper_t *m, std::vector<wm::ReadIn> &reads, double tm0, int slot)
{
	wm_mapper_t::Result &R = m->res[slot];
	static const bool trace_m = getenv("WM_TRACE") != 0;
	const int n = (int)reads.size();
	uint64_t bases = 0;
	for (int i = 0; i < n; ++i) bases += reads[i].seq.size();
	std::vector<wm::ReadOut> out(n);
	const double tm1 = now_ms();
	{
		std::lock_guard<std::mutex> lk(m->stats_mu);
		ensure_ops(m);
	}
	GpuOps &ops = *m->ops;
	uint64_t cells0 = 0; double ksw_us0 = 0, aux_us0 = 0;
	for (GpuOpsCtx &x : ops.ctxs) { cells0 += x.cells; ksw_us0 += x.ksw_us; aux_us0 += x.aux_us; }      // (contexts are shared: this call's share = the difference; approximate when two calls overlap)
	wm::MapStats st;
	hipSetDevice(m->c->device);
	// records are formatted by the worker that finishes a read, while the other reads are still being mapped
	std::vector<std::string> texts(n);
	const std::function<void(size_t)> fmt = [&](size_t i) { wm::write_read(texts[i], m->idx->ix, reads[i], out[i], m->mo.flag); };
	CallOps call(ops);                       // this call's view of the shared contexts: its failed batches fail this call, nobody else's
	wm::map_batch(m->idx->ix, m->mo, &call, reads, out, &st, m->call_threads(), &fmt, slot);
	if (!call.err.msg.empty()) return set_err(WM_ENODEV, "%s", call.err.msg.c_str());
	if (!st.internal_error.empty()) return set_err(WM_EINTERNAL, "%s", st.internal_error.c_str());
	{ std::string ie; if (wm::take_internal_error(ie)) return set_err(WM_EINTERNAL, "%s", ie.c_str()); }      // (recorded by a thread outside any call's team)
	GpuOpsCtx tot; tot.c = m->c;
	for (GpuOpsCtx &x : ops.ctxs) { tot.cells += x.cells; tot.ksw_us += x.ksw_us; tot.aux_us += x.aux_us; }
	tot.cells -= cells0; tot.ksw_us -= ksw_us0; tot.aux_us -= aux_us0;
	GpuOpsCtx &opsr = tot;
	if (getenv("WM_TRACE")) {
		double a[8] = {0};
		for (GpuOpsCtx &x : ops.ctxs) { a[0] += x.t_pack; a[1] += x.t_prep; a[2] += x.t_run; a[3] += x.t_fetch; a[4] += x.t_unpack; a[5] += x.t_sketch; a[6] += x.t_seed; a[7] += x.t_chain; }
		fprintf(stderr, "[ops, sum over %zu contexts, ms] ksw: pack %.0f prepare %.0f run %.0f fetch %.0f unpack %.0f | sketch %.0f seed %.0f chain %.0f | batches %llu\n", ops.ctxs.size(), a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], (unsigned long long)st.n_flush);
	}
	const double tm2 = now_ms();
	// output records (formatted above, per read), laid out in input order
	std::vector<size_t> toff(n + 1, 0), coff(n + 1, 0);
	R.first.assign(n + 1, 0);
	R.rl_defined.resize(n);
	for (int i = 0; i < n; ++i) {
		R.rl_defined[i] = out[i].rep_len_defined ? 1 : 0;
		toff[i + 1] = toff[i] + texts[i].size();
		R.first[i + 1] = R.first[i] + (int64_t)out[i].regs.size();
		size_t nc = 0;
		for (const wm::Reg &r : out[i].regs) nc += r.cigar.size();
		coff[i + 1] = coff[i] + nc;
	}
	R.text.resize(toff[n]); R.hits.resize((size_t)R.first[n] * 16); R.cigars.resize(coff[n]);
	wm::parallel_for(m->n_threads, (size_t)n, [&](size_t i) {
		if (!texts[i].empty()) memcpy(&R.text[toff[i]], texts[i].data(), texts[i].size());
		int32_t *ho = R.hits.data() + (size_t)R.first[i] * 16;
		uint32_t *co = R.cigars.data() + coff[i];
		for (const wm::Reg &r : out[i].regs) {
			const int32_t o[16] = { r.rid, r.rs, r.re, r.qs, r.qe, (int32_t)r.rev, (int32_t)r.mapq, r.has_p ? (int32_t)r.cigar.size() : 0, r.score, r.cnt, r.mlen, r.blen,
			                        r.dp_score, r.dp_max, r.dp_max2, (int32_t)((r.parent == r.id) | r.inv << 1 | r.sam_pri << 2 | r.split << 3 | (r.has_p ? r.trans_strand << 5 : 0)) };
			memcpy(ho, o, sizeof(o)); ho += 16;
			if (!r.cigar.empty()) { memcpy(co, r.cigar.data(), r.cigar.size() * 4); co += r.cigar.size(); }
		}
	});
	if (trace_m) fprintf(stderr, "[map_reads] n=%d ingest %.1f ms, map %.1f ms, format %.1f ms\n", n, tm1 - tm0, tm2 - tm1, now_ms() - tm2);
	std::lock_guard<std::mutex> stats_lk(m->stats_mu);
	m->stats[0] = st.n_flush; m->stats[1] = st.n_ksw; m->stats[2] = st.n_chain; m->stats[3] = st.n_seed; m->stats[4] = st.n_sketch;
	m->host_stats[0] += st.cpu_fiber; m->host_stats[1] += st.wall_idle;
	for (int op = 0; op < 4; ++op) { m->host_stats[2 + op] += st.cpu_op[op]; m->host_stats[6 + op] += st.wall_op[op]; m->host_stats[10 + op] += (double)st.n_batches[op]; }
	m->host_stats[14] += (tm2 - tm1) * 1e-3; m->host_stats[15] += (now_ms() - tm2) * 1e-3; m->host_stats[16] = m->call_threads(); m->host_stats[17] += st.cpu_help;
	m->host_stats[18] += st.wall_fiber; m->host_stats[19] += st.wall_lock; m->host_stats[20] += st.wall_total;
	if (trace_m) fprintf(stderr, "[host] fibers cpu %.2f s | idle wall %.2f s | batched calls cpu/wall/n: sketch %.2f/%.2f/%llu seed %.2f/%.2f/%llu chain %.2f/%.2f/%llu ksw %.2f/%.2f/%llu\n", st.cpu_fiber, st.wall_idle,
	                     st.cpu_op[0], st.wall_op[0], (unsigned long long)st.n_batches[0], st.cpu_op[1], st.wall_op[1], (unsigned long long)st.n_batches[1],
	                     st.cpu_op[2], st.wall_op[2], (unsigned long long)st.n_batches[2], st.cpu_op[3], st.wall_op[3], (unsigned long long)st.n_batches[3]);
	m->stats[5] = opsr.cells; m->stats[6] = (uint64_t)opsr.ksw_us; m->stats[7] = (uint64_t)opsr.aux_us; m->stats[8] = bases;
	return WM_OK;
}

// The file-level loop (mm_map_file, src/map.c:1226-1268): reads FASTA/FASTQ(.gz) mini-batches of `mini_batch_bases` (0 = the
// reference's default 1 Gbase), maps them and writes the records to out_path ("-" = stdout), reader / mapper / writer
// overlapped. Every mini-batch is ordered like the reference orders it, so the file equals the reference's output.
// stats (optional, 6 doubles): reads, bases, batches, seconds spent reading / mapping / writing.
// the command line for the @PG line of wm_map_file_split (no mapper object outlives its parts); wm_mapper_set_cmdline stores it here as well
static std::mutex g_cmdline_mu;
static std::vector<std::string> g_cmdline;
static bool g_split_pg = true;              // wm_map_file_split prints the @PG line itself
extern "C" int wm_set_cmdline(int argc, const char *const *argv)
{
	if (argc > 0 && !argv) return set_err(WM_EINVAL, "bad argument");
	std::lock_guard<std::mutex> lk(g_cmdline_mu);
	g_split_pg = argc >= 0;                  // argc < 0: the front end has printed @PG already (the reference's main does, src/main.c:395)
	g_cmdline.clear();
	if (argc > 0) g_cmdline.assign(argv, argv + argc);
	return WM_OK;
}
extern "C" int wm_mapper_set_cmdline(wm_mapper_t *m, int argc, const char *const *argv)
{
	if (!m || argc < 0 || (argc > 0 && !argv)) return set_err(WM_EINVAL, "bad argument");
	m->cmdline.assign(argv, argv + argc);
	return WM_OK;
}

// wm_last_error is per thread and the second mapping lane of the file loops is a thread of its own: a lane keeps the code and message of its
// failed call here and the entry point re-issues them on the caller's thread (ENODEV / ENOMEM of lane 1 used to surface as "mapping failed")
struct LaneError {
	std::mutex mu; int code = 0; std::string msg;
	void keep(int rc) { std::lock_guard<std::mutex> lk(mu); if (!code) { code = rc; msg = wm_err_text(); } }
};

extern "C" int wm_map_file(wm_mapper_t *m, const char *reads_path, const char *out_path, int64_t mini_batch_bases, double *stats)
{
	wm_err_clear();
	FILE *out = strcmp(out_path, "-") == 0 ? stdout : fopen(out_path, "wb");
	if (!out) return set_err(WM_EINVAL, "cannot open '%s' for writing", out_path);
	std::string err;
	if ((m->mo.flag & 0x8) && m->sam_header) {                         // MM_F_OUT_SAM: @SQ / @PG lines first (mm_write_sam_hdr, src/main.c:393)
		std::string hdr;
		std::vector<const char*> av;
		for (const std::string &a : m->cmdline) av.push_back(a.c_str());
		wm::write_sam_header(hdr, m->idx->ix, (int)av.size(), av.data());
		if (fwrite(hdr.data(), 1, hdr.size(), out) != hdr.size()) { if (out != stdout) fclose(out); return set_err(WM_EINVAL, "write error on '%s'", out_path); }
	}
	wm::FileStats fs;
	const bool with_qual = (m->mo.flag & 0x8) != 0;                    // SAM output prints QUAL
	LaneError le;
	const int rc = wm::map_file(reads_path, mini_batch_bases, with_qual, [&](std::vector<wm::ReadIn> &batch, std::string &text, int lane) {
		const int r = map_reads_impl(m, batch, now_ms(), lane);             // (WM_MAP_LANES mini-batches in flight, default 2: lane = result slot = slab of resident read codes)
		if (r == 0) text.swap(m->res[lane].text);
		else le.keep(r);
		return r;
	}, out, &fs, err);
	if (out != stdout) fclose(out);
	if (stats) { stats[0] = (double)fs.n_reads; stats[1] = (double)fs.n_bases; stats[2] = (double)fs.n_batches; stats[3] = fs.t_read; stats[4] = fs.t_map; stats[5] = fs.t_write; }
	if (rc) return le.code ? set_err(le.code, "%s", le.msg.c_str()) : set_err(WM_EINVAL, "%s", err.c_str());
	return WM_OK;
}

// The file loop over N mappers — one per GPU of the node (each with its own context, index copy and host threads: wm_ctx_create(device i),
// wm_index_upload_peer, wm_mapper_create, wm_mapper_set_threads) — inside ONE process: the C twin of `one rank per GPU`. The reader hands mini-batches
// to WM_MAP_LANES (default 2) lanes per mapper (lane l -> mapper l % n, result slot l / n), reads shard by mini-batch, nothing is exchanged between the devices, and the
// ordered writer puts the records back into input order: the output file equals wm_map_file's (and the reference's). The SAM header, if wanted, is
// written once from the first mapper's index and command line.
extern "C" int wm_map_file_multi(wm_mapper_t *const *ms, int n, const char *reads_path, const char *out_path, int64_t mini_batch_bases, double *stats)
{
	wm_err_clear();
	if (!ms || n < 1 || !reads_path || !out_path) return set_err(WM_EINVAL, "bad argument");
	for (int i = 0; i < n; ++i) {
		if (!ms[i]) return set_err(WM_EINVAL, "null mapper");
		if (ms[i]->mo.flag != ms[0]->mo.flag || ms[i]->idx->ix.seq.size() != ms[0]->idx->ix.seq.size() || ms[i]->idx->ix.hbits != ms[0]->idx->ix.hbits)
			return set_err(WM_EINVAL, "mapper %d differs from mapper 0 (options or index)", i);
	}
	FILE *out = strcmp(out_path, "-") == 0 ? stdout : fopen(out_path, "wb");
	if (!out) return set_err(WM_EINVAL, "cannot open '%s' for writing", out_path);
	wm_mapper_t *m0 = ms[0];
	std::string err;
	if ((m0->mo.flag & 0x8) && m0->sam_header) {
		std::string hdr;
		std::vector<const char*> av;
		for (const std::string &a : m0->cmdline) av.push_back(a.c_str());
		wm::write_sam_header(hdr, m0->idx->ix, (int)av.size(), av.data());
		if (fwrite(hdr.data(), 1, hdr.size(), out) != hdr.size()) { if (out != stdout) fclose(out); return set_err(WM_EINVAL, "write error on '%s'", out_path); }
	}
	wm::FileStats fs;
	const bool with_qual = (m0->mo.flag & 0x8) != 0;
	LaneError le;
	// n mappers x lanes mapping calls run at once, each with its mapper's worker threads: on a host whose usable cores (affinity, cgroup quota) are fewer
	// than that product the calls are given an equal share each for the duration of the loop (eight mappers of sixteen threads under a 16-CPU quota were
	// 256 runnable threads: the collapse of profiles/r04j). WM_MULTI_THREADS=<n> sets the share per call, 0 leaves the mappers' own counts.
	{
		const int lanes = wm::default_lanes() * n;
		int share = wm::usable_cores() / lanes;
		if (getenv("WM_MULTI_THREADS")) share = atoi(getenv("WM_MULTI_THREADS"));
		else if (share < 2) share = 2;
		for (int i = 0; i < n; ++i) ms[i]->n_threads_cap = n > 1 ? share : 0;
	}
	struct Uncap { wm_mapper_t *const *ms; int n; ~Uncap() { for (int i = 0; i < n; ++i) ms[i]->n_threads_cap = 0; } } uncap{ ms, n };
	const int rc = wm::map_file(reads_path, mini_batch_bases, with_qual, [&](std::vector<wm::ReadIn> &batch, std::string &text, int lane) {
		wm_mapper_t *m = ms[lane % n];
		const int slot = lane / n;
		const int r = map_reads_impl(m, batch, now_ms(), slot);
		if (r == 0) text.swap(m->res[slot].text);
		else le.keep(r);
		return r;
	}, out, &fs, err, wm::default_lanes() * n);
	if (out != stdout) fclose(out);
	if (stats) { stats[0] = (double)fs.n_reads; stats[1] = (double)fs.n_bases; stats[2] = (double)fs.n_batches; stats[3] = fs.t_read; stats[4] = fs.t_map; stats[5] = fs.t_write; }
	if (rc) return le.code ? set_err(le.code, "%s", le.msg.c_str()) : set_err(WM_EINVAL, "%s", err.c_str());
	return WM_OK;
}

// ---- a reference indexed in parts (-I, --split-prefix; src/main.c:398-429, src/map.c:1050-1105, src/splitidx.c) ----
extern "C" int wm_index_build_parts(const char *fasta, const char *kmer_file, int k, int w, int n_threads, uint64_t batch_bases, wm_index_t **out, int cap, int *n_parts)
{
	if (!fasta || !out || !n_parts || cap < 1 || batch_bases == 0) return set_err(WM_EINVAL, "bad argument");
	*n_parts = 0;
	wm::IdxOpt io; io.k = k; io.w = w;
	wm::MapOpt mo; std::string err;
	if (wm::check_opt(io, mo, err) < 0) return set_err(WM_EINVAL, "%s", err.c_str());
	std::vector<wm::Index> parts;
	const int n = wm::index_build_parts_from_fasta(io, fasta, kmer_file ? kmer_file : "", n_threads, batch_bases, parts, err);
	if (n < 0) return set_err(WM_EINVAL, "%s", err.c_str());
	if (n > cap) return set_err(WM_ENOMEM, "the reference has %d index parts, room for %d", n, cap);
	for (int i = 0; i < n; ++i) { out[i] = new wm_index_t(); out[i]->ix = std::move(parts[i]); }
	*n_parts = n;
	return WM_OK;
}

// one mini-batch against the mapper's index, hits kept as they are (no records)
static int map_reads_raw(wm_mapper_t *m, std::vector<wm::ReadIn> &reads, std::vector<wm::ReadOut> &out, int slot)
{
	{
		std::lock_guard<std::mutex> lk(m->stats_mu);
		ensure_ops(m);
	}
	GpuOps &ops = *m->ops;
	wm::MapStats st;
	hipSetDevice(m->c->device);
	CallOps call(ops);
	wm::map_batch(m->idx->ix, m->mo, &call, reads, out, &st, m->n_threads, 0, slot);
	if (!call.err.msg.empty()) return set_err(WM_ENODEV, "%s", call.err.msg.c_str());
	if (!st.internal_error.empty()) return set_err(WM_EINTERNAL, "%s", st.internal_error.c_str());
	{ std::string ie; if (wm::take_internal_error(ie)) return set_err(WM_EINTERNAL, "%s", ie.c_str()); }
	return WM_OK;
}

// One part at a time (src/main.c:398-429: the reference's main holds one mm_idx_t, maps every read against it, destroys it, reads the next): wm_split_begin,
// wm_split_add_part per part — upload, mapper, the whole reads file against it, hits spilled; the part may be destroyed on return —, wm_split_finish = header + merge.
struct wm_split_s {
	wm_ctx_t *c; wm_mapopt_t copt; wm::MapOpt mo; int n_threads; int k, w;
	wm::SplitRun *run;
};
extern "C" int wm_split_begin(wm_ctx_t *c, const wm_mapopt_t *opt, int k, int w, int n_threads, const char *reads_path, int64_t mini_batch_bases, wm_split_t **out)
{
	wm_err_clear();
	if (!c || !opt || !reads_path || !out) return set_err(WM_EINVAL, "bad argument");
	*out = 0;
	wm::MapOpt mo; wm::IdxOpt io;
	wm::set_preset(0, io, mo);
	mapopt_from_c(opt, mo);
	if (mo.flag & (wm::F_OUT_CS | wm::F_OUT_MD)) return set_err(WM_EINVAL, "--cs or --MD doesn't work with a reference indexed in parts");      // src/options.c:139-141
	wm_split_t *s = new wm_split_t();
	s->c = c; s->copt = *opt; s->mo = mo; s->n_threads = n_threads > 1 ? n_threads : 1; s->k = k; s->w = w;
	s->run = new wm::SplitRun(reads_path, mini_batch_bases, mo, k, w);
	*out = s;
	return WM_OK;
}
extern "C" void wm_split_abort(wm_split_t *s) { if (s) { delete s->run; delete s; } }
extern "C" int wm_split_add_part(wm_split_t *s, wm_index_t *part)
{
	wm_err_clear();
	if (!s || !part) return set_err(WM_EINVAL, "null argument");
	if (part->ix.k != s->k || part->ix.w != s->w) return set_err(WM_EINVAL, "index part built with k = %d, w = %d; the run was started for k = %d, w = %d", part->ix.k, part->ix.w, s->k, s->w);
	wm_mapper_t *m = 0;
	int rc0;
	if ((rc0 = wm_index_upload(s->c, part)) != WM_OK) return rc0;                       // (the message is the failing call's)
	if ((rc0 = wm_mapper_create_opt(s->c, part, &s->copt, &m)) != WM_OK) return rc0;
	if ((rc0 = wm_mapper_set_threads(m, s->n_threads, 0)) != WM_OK) { wm_mapper_destroy(m); return rc0; }
	LaneError le;
	std::string err;
	const int rc = s->run->add_part(part->ix.seq, [&](std::vector<wm::ReadIn> &batch, std::vector<wm::ReadOut> &o, int lane) -> int { const int r = map_reads_raw(m, batch, o, lane); if (r) le.keep(r); return r; }, err);
	wm_mapper_destroy(m);
	if (rc) return le.code ? set_err(le.code, "%s", le.msg.c_str()) : set_err(WM_EINVAL, "%s", err.c_str());
	return WM_OK;
}
extern "C" int wm_split_finish(wm_split_t *s, const char *out_path, double *stats)
{
	wm_err_clear();
	if (!s || !out_path) { wm_split_abort(s); return set_err(WM_EINVAL, "bad argument"); }
	FILE *out = strcmp(out_path, "-") == 0 ? stdout : fopen(out_path, "wb");
	if (!out) { wm_split_abort(s); return set_err(WM_EINVAL, "cannot open '%s' for writing", out_path); }
	if (s->mo.flag & 0x8) {
		// SAM: the reference's main prints @PG (with CL:) when it sees the first of several parts (mm_write_sam_hdr(0, ...), src/main.c:395); the merge
		// pass then lists every part's contigs (src/map.c:1304-1306) — @PG first, @SQ after it
		std::string hdr, sq;
		wm::Index none;
		std::vector<const char*> av;
		bool with_pg;
		{ std::lock_guard<std::mutex> lk(g_cmdline_mu); for (const std::string &a : g_cmdline) av.push_back(a.c_str()); with_pg = g_split_pg; }
		if (with_pg) wm::write_sam_header(hdr, none, (int)av.size(), av.data());
		wm::write_sam_header(sq, s->run->dict(), 0, 0);
		hdr += sq.substr(0, sq.rfind("@PG"));
		if (fwrite(hdr.data(), 1, hdr.size(), out) != hdr.size()) { if (out != stdout) fclose(out); wm_split_abort(s); return set_err(WM_EINVAL, "write error on '%s'", out_path); }
	}
	wm::FileStats fs;
	std::string err;
	const int rc = s->run->finish(out, &fs, err);
	if (out != stdout) fclose(out);
	if (stats) { stats[0] = (double)fs.n_reads; stats[1] = (double)fs.n_bases; stats[2] = (double)fs.n_batches; stats[3] = fs.t_read; stats[4] = fs.t_map; stats[5] = fs.t_write; }
	wm_split_abort(s);
	if (rc) return set_err(WM_EINVAL, "%s", err.c_str());
	return WM_OK;
}

// every part given up front (rounds 3-4; the parts stay the caller's)
extern "C" int wm_map_file_split(wm_ctx_t *c, int n_parts, wm_index_t *const *parts, const wm_mapopt_t *opt, int n_threads, const char *reads_path, const char *out_path,
                                 int64_t mini_batch_bases, double *stats)
{
	wm_err_clear();
	if (!c || n_parts < 1 || !parts || !opt || !reads_path || !out_path) return set_err(WM_EINVAL, "bad argument");
	for (int j = 0; j < n_parts; ++j) if (!parts[j]) return set_err(WM_EINVAL, "null index part");
	wm_split_t *s = 0;
	int rc = wm_split_begin(c, opt, parts[0]->ix.k, parts[0]->ix.w, n_threads, reads_path, mini_batch_bases, &s);
	if (rc) return rc;
	for (int j = 0; j < n_parts; ++j)
		if ((rc = wm_split_add_part(s, parts[j])) != WM_OK) { wm_split_abort(s); return rc; }
	return wm_split_finish(s, out_path, stats);
}

// the reference FASTA indexed part by part AS THE RUN GOES: one part in host memory (and one on the device) at a time, like `winnowmap -I <batch_bases>
// --split-prefix` (src/main.c:417-419). on_device: the part's minimizers are sketched and its table built on the GPU (wm_index_build_dev's path).
extern "C" int wm_map_file_split_fasta(wm_ctx_t *c, const char *fasta, const char *kmer_file, int k, int w, int build_threads, uint64_t batch_bases, int on_device,
                                       const wm_mapopt_t *opt, int n_threads, const char *reads_path, const char *out_path, int64_t mini_batch_bases, double *stats, int *n_parts)
{
	wm_err_clear();
	if (!c || !fasta || !opt || !reads_path || !out_path || batch_bases == 0) return set_err(WM_EINVAL, "bad argument");
	if (n_parts) *n_parts = 0;
	wm::IdxOpt io; io.k = k; io.w = w;
	{ wm::MapOpt mo; std::string e; if (wm::check_opt(io, mo, e) < 0) return set_err(WM_EINVAL, "%s", e.c_str()); }
	wm::IndexPartReader rd;
	std::string err;
	if (rd.open(fasta, err) < 0) return set_err(WM_EINVAL, "%s", err.c_str());
	wm_split_t *s = 0;
	int rc = wm_split_begin(c, opt, k, w, n_threads, reads_path, mini_batch_bases, &s);
	if (rc) return rc;
	std::vector<std::string> names, seqs;
	int n = 0;
	while (rd.next(batch_bases, names, seqs) > 0) {
		wm_index_t *part = 0;
		if (on_device) rc = wm_index_build_seqs_dev(c, io, names, seqs, kmer_file ? kmer_file : "", build_threads, &part);
		else {
			part = new wm_index_t();
			if (wm::index_build(io, names, seqs, kmer_file ? kmer_file : "", build_threads, part->ix, err) < 0) { delete part; part = 0; rc = set_err(WM_EINVAL, "%s", err.c_str()); }
		}
		std::vector<std::string>().swap(seqs);
		if (rc == WM_OK) rc = wm_split_add_part(s, part);
		if (part) wm_index_destroy(part);
		if (rc) { wm_split_abort(s); return rc; }
		++n;
	}
	if (n == 0) { wm_split_abort(s); return set_err(WM_EINVAL, "no sequences in %s", fasta); }
	if (n_parts) *n_parts = n;
	return wm_split_finish(s, out_path, stats);
}

extern "C" int wm_index_read_junc_bed(wm_index_t *idx, const char *path)
{
	if (!idx || !path) return set_err(WM_EINVAL, "null argument");
	std::string err;
	if (wm::index_read_bed(idx->ix, path, true, err) < 0) return set_err(WM_EINVAL, "%s", err.c_str());
	return WM_OK;
}
extern "C" int wm_index_add_junc(wm_index_t *idx, int ctg, int n, const int32_t *st, const int32_t *en, const int32_t *strand)
{
	if (!idx || ctg < 0 || ctg >= (int)idx->ix.seq.size() || n < 0 || (n > 0 && (!st || !en || !strand))) return set_err(WM_EINVAL, "bad argument");
	if (idx->ix.I.empty()) idx->ix.I.resize(idx->ix.seq.size());
	std::vector<wm::JuncIntv> &r = idx->ix.I[ctg];
	for (int i = 0; i < n; ++i) r.push_back(wm::JuncIntv{ st[i], en[i], strand[i] });
	std::stable_sort(r.begin(), r.end(), [](const wm::JuncIntv &a, const wm::JuncIntv &b) { return a.st < b.st; });
	return WM_OK;
}

extern "C" int wm_ksw_ll_i16(int qlen, const uint8_t *query, int tlen, const uint8_t *target, const int8_t *mat5x5, int gapo, int gape, int *qe, int *te)
{
	int q = -1, t = -1;
	const int sc = wm::ll_i16(qlen, query, tlen, target, mat5x5, gapo, gape, &q, &t);
	if (qe) *qe = q;
	if (te) *te = t;
	return sc;
}

extern "C" int wm_ksw_n_classes(void) { return WM_KSW_NCLASS; }      // kernel classes wm_mapper_kernel_stats / _union report on (ksw_plan.h)
extern "C" int wm_mapper_stats(const wm_mapper_t *m, uint64_t *out9) { memcpy(out9, m->stats, sizeof(m->stats)); return WM_OK; }
// per ksw kernel class (ksw_plan.h) since the mapper was created: out[3*k] = summed launch durations in ms (HIP events on the
// launching stream), out[3*k+1] = DP cells, out[3*k+2] = launches; n_classes receives WM_KSW_NCLASS
extern "C" int wm_mapper_kernel_stats(const wm_mapper_t *m, double *out, int cap, int *n_classes)
{
	if (n_classes) *n_classes = WM_KSW_NCLASS;
	if (cap < 3 * WM_KSW_NCLASS) return set_err(WM_EINVAL, "need room for %d doubles", 3 * WM_KSW_NCLASS);
	for (int k = 0; k < WM_KSW_NCLASS; ++k) {
		double ms = m->c->k_ms[k], cells = (double)m->c->k_cells[k], ln = (double)m->c->k_launches[k];
		for (const wm_ctx_t *w : m->workers) { ms += w->k_ms[k]; cells += (double)w->k_cells[k]; ln += (double)w->k_launches[k]; }
		out[3 * k] = ms; out[3 * k + 1] = cells; out[3 * k + 2] = ln;
	}
	return WM_OK;
}

// out[k] = milliseconds during which at least one launch of ksw class k was running (union of its launch intervals over all contexts), counting
// only what lies after `since_ms` on the device clock; returns through *now_ms the current reading of that clock (pass it as since_ms next time)
extern "C" int wm_mapper_kernel_union(const wm_mapper_t *m, double since_ms, double *out, int cap, double *now_ms_out)
{
	if (!m || cap < WM_KSW_NCLASS) return set_err(WM_EINVAL, "need room for %d doubles", WM_KSW_NCLASS);
	std::vector<const wm_ctx_t*> cs; cs.push_back(m->c); cs.insert(cs.end(), m->workers.begin(), m->workers.end());
	for (int k = 0; k < WM_KSW_NCLASS; ++k) {
		std::vector<std::pair<float, float>> iv;
		for (const wm_ctx_t *c : cs) {
			std::lock_guard<std::mutex> lk(const_cast<wm_ctx_t*>(c)->iv_mu);
			for (const auto &p : c->k_iv[k]) if (p.second > since_ms) iv.push_back(std::make_pair(std::max(p.first, (float)since_ms), p.second));
		}
		std::sort(iv.begin(), iv.end());
		double tot = 0, cur_s = 0, cur_e = -1;
		for (const auto &p : iv) {
			if (p.first > cur_e) { if (cur_e > cur_s) tot += cur_e - cur_s; cur_s = p.first; cur_e = p.second; }
			else if (p.second > cur_e) cur_e = p.second;
		}
		if (cur_e > cur_s) tot += cur_e - cur_s;
		out[k] = tot;
	}
	if (now_ms_out) {
		*now_ms_out = 0;
		hipEvent_t base = device_base_event(m->c->device), e;
		if (base && hipEventCreate(&e) == hipSuccess) {
			float t = 0;
			if (hipEventRecord(e, m->c->stream) == hipSuccess && hipEventSynchronize(e) == hipSuccess && hipEventElapsedTime(&t, base, e) == hipSuccess) *now_ms_out = t;
			hipEventDestroy(e);
		}
	}
	return WM_OK;
}

extern "C" int wm_mapper_host_stats(const wm_mapper_t *m, double *out, int cap)
{
	if (cap < 18) return set_err(WM_EINVAL, "need room for 18 doubles");
	memcpy(out, m->host_stats, (size_t)(cap < 24 ? cap : 24) * sizeof(double));
	return WM_OK;
}

extern "C" int wm_sam_header(const wm_index_t *idx, int argc, const char *const *argv, const char **text, size_t *text_len)
{
	static thread_local std::string s;
	s.clear();
	wm::write_sam_header(s, idx->ix, argc, argv);
	*text = s.data(); *text_len = s.size();
	return WM_OK;
}


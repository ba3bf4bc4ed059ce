// tests/host_harness/harness.cpp — TEST INFRASTRUCTURE ONLY.
// Drives the product's HOST mapper (winnowmap_amd/csrc/host/*.cpp: index, MCAS fibers, hit/align glue) with a
// DeviceOps implementation backed by the ORACLE (oracle/wm_oracle.c), so that the host logic can be compared with
// the real reference end-to-end on a machine without a GPU. The product never links this file.
#include "../../winnowmap_amd/csrc/host/wm_core.cpp"
#include "../../winnowmap_amd/csrc/host/wm_index.cpp"
#include "../../winnowmap_amd/csrc/host/wm_seqio.cpp"
#include "../../winnowmap_amd/csrc/host/wm_hit.cpp"
#include "../../winnowmap_amd/csrc/host/wm_align.cpp"
#include "../../winnowmap_amd/csrc/host/wm_mapper.cpp"
#include "../../winnowmap_amd/csrc/host/wm_chain.cpp"
#include "../../winnowmap_amd/csrc/host/wm_ops.cpp"
#include "../../winnowmap_amd/csrc/host/wm_format.cpp"
#include "../../winnowmap_amd/csrc/host/wm_pipeline.cpp"
#include "../../oracle/wm_oracle.h"
#include "../../winnowmap_amd/csrc/reads2bit.h"
#include "../../winnowmap_amd/csrc/host/wm_final_plan.h"
#include <fstream>
#include <set>
#include <stdexcept>
#include <stdarg.h>

using namespace wm;

struct OracleOps : DeviceOps {
	const Index *idx; wmo_bloom_t *bloom; const MapOpt *opt;
	int max_inflight() const override { return 64; }             // stateless CPU calls: any number may run at once
	// "resident" data like the device implementation keeps it: the batch's read codes (and the index's packed reference). Requests are
	// served from their host views; the resident positions they carry are decoded as well and must give the same bytes.
	// (kept the way the device keeps them: 2 bits per base + an ambiguity bitmap, packed by the product's wm_pack_codes — csrc/reads2bit.h)
	// One slab per slot, like the device's (two mapping calls may be in flight on one ops object: wm_map_file's lanes); a call's offsets start at slot * SLAB.
	static constexpr int64_t SLAB = (int64_t)1 << 40;
	std::vector<uint64_t> rd_pk[4], rd_nm[4]; size_t rd_n[4] = { 0, 0, 0, 0 };
	std::atomic<long> n_pos_checked{0}, n_pos_bad{0};
	bool load_reads(const uint8_t *codes, size_t n, int slot, int64_t *base) override
	{
		if (slot < 0 || slot >= 4) { *base = 0; return false; }
		rd_pk[slot].assign(wm_pk_words(n), ~0ULL); rd_nm[slot].assign(wm_nm_words(n), ~0ULL);
		wm_pack_codes(codes, n, rd_pk[slot].data(), rd_nm[slot].data());
		rd_n[slot] = n; *base = (int64_t)slot * SLAB;
		return true;
	}
	bool rd_in(int64_t p, int64_t len) const { const int64_t sl = p / SLAB, o = p % SLAB; return p >= 0 && sl < 4 && (size_t)(o + len) <= rd_n[sl]; }
	uint8_t rd_at(int64_t p) const { const int64_t sl = p / SLAB; return (uint8_t)wm_rd_code(rd_pk[sl].data(), rd_nm[sl].data(), (uint64_t)(p % SLAB)); }
	uint8_t two_strand(const KswReq &r, int64_t p) const
	{   // KswReq: [0,L) forward strand, [L,2L) reverse complement, negative = N padding
		const int64_t L = r.qwin_len;
		if (p < 0 || p >= 2 * L) return 4;
		const uint8_t c = p < L ? rd_at(r.qwin_off + p) : rd_at(r.qwin_off + (2 * L - 1 - p));
		return p < L ? c : (c < 4 ? 3 - c : 4);
	}
	void check_positions(const KswReq &r, const std::vector<uint8_t> &q, const std::vector<uint8_t> &t)
	{
		if (!r.resident()) return;
		bool bad = false, any_n = false;
		for (int i = 0; i < r.ql; ++i) { bad |= two_strand(r, (int64_t)r.q_pos + (int64_t)i * r.step) != q[i]; any_n |= q[i] >= 4; }
		std::vector<uint8_t> tt(r.tl > 0 ? r.tl : 0);
		if (r.tl > 0) {
			const int lo = r.step > 0 ? r.t_pos : r.t_pos - (r.tl - 1);
			idx->getseq(r.rid, lo, lo + r.tl, tt.data());
			for (int i = 0; i < r.tl; ++i) { bad |= tt[r.step > 0 ? i : r.tl - 1 - i] != t[i]; any_n |= t[i] >= 4; }
		}
		if (any_n && !r.has_n) bad = true;                        // has_n may be conservative, never optimistic
		++n_pos_checked; if (bad) ++n_pos_bad;
	}
	void sketch_batch(int w, int k, std::vector<SketchReq*> &reqs) override
	{
		for (SketchReq *r : reqs) {
			if (r->dev_off >= 0) { ++n_pos_checked; bool bad = !rd_in(r->dev_off, r->len); for (int64_t t = 0; !bad && t < r->len; ++t) bad = rd_at(r->dev_off + t) != r->seq[t]; if (bad) ++n_pos_bad; }
			std::vector<uint64_t> x(r->len + 8), y(r->len + 8);
			int64_t n = (idx->flag & 1 ? wmo_sketch_hpc : wmo_sketch)((const char*)r->seq, r->len, w, k, 0, bloom, x.data(), y.data(), r->len + 8);
			r->mini.resize(n);
			for (int64_t i = 0; i < n; ++i) r->mini[i].x = x[i], r->mini[i].y = y[i];
		}
	}
	void seed_batch(std::vector<SeedReq*> &reqs) override
	{   // collect_matches + collect_seed_hits restated for the test (src/map.c:97-130, 222-254)
		for (SeedReq *r : reqs) {
			int rep_st = 0, rep_en = 0, rep_len = 0;
			std::vector<wmo128_t> a;
			for (int i = 0; i < r->n_mini; ++i) {
				const m128 &p = r->mini[i];
				const uint32_t q_pos = (uint32_t)p.y, q_span = p.x & 0xff;
				int t;
				const uint64_t *cr = idx->get(p.x >> 8, &t);
				if (t >= r->max_occ) {
					int en = (q_pos >> 1) + 1, st = en - q_span;
					if (st > rep_en) { rep_len += rep_en - rep_st; rep_st = st, rep_en = en; } else rep_en = en;
					continue;
				}
				bool tandem = false;
				if (i > 0 && p.x >> 8 == r->mini[i - 1].x >> 8) tandem = true;
				if (i < r->n_mini - 1 && p.x >> 8 == r->mini[i + 1].x >> 8) tandem = true;
				for (int k = 0; k < t; ++k) {
					const uint64_t rr = cr[k];
					const int32_t rpos = (uint32_t)rr >> 1;
					const bool fwd = (rr & 1) == (q_pos & 1);
					if ((r->flag & F_FOR_ONLY) && !fwd) continue;
					if ((r->flag & F_REV_ONLY) && fwd) continue;
					wmo128_t e;
					if (fwd) { e.x = (rr & 0xffffffff00000000ULL) | (uint64_t)rpos; e.y = (uint64_t)q_span << 32 | q_pos >> 1; }
					else { e.x = 1ULL << 63 | (rr & 0xffffffff00000000ULL) | (uint64_t)rpos; e.y = (uint64_t)q_span << 32 | (uint32_t)(r->qlen - ((q_pos >> 1) + 1 - q_span) - 1); }
					if (tandem) e.y |= SEED_TANDEM;
					a.push_back(e);
				}
			}
			rep_len += rep_en - rep_st;
			wmo_radix_sort_128x(a.data(), a.data() + a.size());
			r->a.resize(a.size());
			for (size_t i = 0; i < a.size(); ++i) r->a[i].x = a[i].x, r->a[i].y = a[i].y;
			r->rep_len = rep_len;
		}
	}
	void chain_batch(std::vector<ChainReq*> &reqs) override
	{
		for (ChainReq *r : reqs) {
			const int64_t n = (int64_t)r->a.size();
			std::vector<wmo128_t> b(n ? n : 1);
			std::vector<uint64_t> u(n ? n : 1);
			int n_u = 0;
			if (const char *dp = getenv("WM_CHAIN_DUMP")) {    // probes: append the job (n, 8 ints + gap_scale, anchors) to a file
				FILE *fp = fopen(dp, "ab");
				int64_t hdr[2] = { n, 0 };
				int32_t par[10] = { r->max_dist_x, r->min_dist_x, r->max_dist_y, r->bw, r->max_skip, r->max_iter, r->min_cnt, r->min_sc, 0, 0 };
				memcpy(&par[8], &r->gap_scale, 4);
				fwrite(hdr, 8, 2, fp); fwrite(par, 4, 10, fp); fwrite(r->a.data(), 16, n, fp); fclose(fp);
			}
			extern int64_t wmo_chain_stat[4];
			wmo_chain_stat[0] = wmo_chain_stat[1] = wmo_chain_stat[2] = wmo_chain_stat[3] = 0;
			wmo_chain_set_cdna(r->is_cdna ? 1 : 0);
			int64_t n_v = wmo_chain_dp(r->max_dist_x, r->min_dist_x, r->max_dist_y, r->bw, r->max_skip, r->max_iter, r->min_cnt, r->min_sc, r->gap_scale,
			                           n, (const wmo128_t*)r->a.data(), &n_u, u.data(), b.data());
			if (getenv("WM_CHAIN_STATS")) fprintf(stderr, "CHAINJOB %lld %lld %lld %lld %lld\n", (long long)n, (long long)wmo_chain_stat[0], (long long)wmo_chain_stat[1], (long long)wmo_chain_stat[2], (long long)wmo_chain_stat[3]);
			r->u.assign(u.begin(), u.begin() + n_u);
			r->a.resize(n_v);
			for (int64_t i = 0; i < n_v; ++i) r->a[i].x = b[i].x, r->a[i].y = b[i].y;
		}
	}
	void ksw_batch(const wm_ksw_score_t &sc, std::vector<KswReq*> &reqs) override
	{
		int8_t mat[25];
		for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) mat[i * 5 + j] = (i == 4 || j == 4) ? sc.sc_ambi : i == j ? sc.match : sc.mismatch;
		wm::parallel_for(4, reqs.size(), [&](size_t ri) {
			KswReq *r = reqs[ri];
			wmo_ez_t ez;
			if (getenv("WM_KSW_STATS")) fprintf(stderr, "KSWJOB %d %d %d %d %d\n", r->ql, r->tl, r->w, r->zdrop, r->flag);
			std::vector<uint8_t> q(r->ql > 0 ? r->ql : 0), t(r->tl > 0 ? r->tl : 0);
			r->copy_query(q.data()); r->copy_target(t.data());
			check_positions(*r, q, t);
			if (const char *dp = getenv("WM_DUMP_KSW")) {        // real alignment jobs of a mapping run, for replays through the kernel emulator
				static std::mutex mu;
				std::lock_guard<std::mutex> lk(mu);
				if (FILE *f = fopen(dp, "ab")) {
					const int32_t hdr[10] = { (int32_t)q.size(), (int32_t)t.size(), r->w, r->zdrop, r->end_bonus, r->flag, sc.match, sc.mismatch, sc.q | sc.e << 8 | sc.q2 << 16 | sc.e2 << 24, sc.sc_ambi };
					fwrite(hdr, 4, 10, f); fwrite(q.data(), 1, q.size(), f); fwrite(t.data(), 1, t.size(), f);
					fclose(f);
				}
			}
			std::vector<uint32_t> cig(q.size() + t.size() + 4);
			wmo_ksw_extd2((int)q.size(), q.data(), (int)t.size(), t.data(), 5, mat, sc.q, sc.e, sc.q2, sc.e2, r->w, r->zdrop, r->end_bonus, r->flag, &ez, cig.data(), 0);
			r->ez.max = ez.max; r->ez.zdropped = ez.zdropped; r->ez.max_q = ez.max_q; r->ez.max_t = ez.max_t; r->ez.mqe = ez.mqe; r->ez.mqe_t = ez.mqe_t;
			r->ez.mte = ez.mte; r->ez.mte_q = ez.mte_q; r->ez.score = ez.score; r->ez.reach_end = ez.reach_end; r->ez.n_cigar = ez.n_cigar; r->ez.cig_off = 0;
			r->cigar.assign(cig.begin(), cig.begin() + ez.n_cigar);
		});
	}
	void exts2_batch(const wm_ksw_score_t &sc, int noncan, int junc_bonus, std::vector<KswReq*> &reqs) override
	{   // splice mode: ksw_exts2_sse per request (src/align.c:326-327)
		int8_t mat[25];
		for (int i = 0; i < 5; ++i) for (int j = 0; j < 5; ++j) mat[i * 5 + j] = (i == 4 || j == 4) ? sc.sc_ambi : i == j ? sc.match : sc.mismatch;
		wm::parallel_for(4, reqs.size(), [&](size_t ri) {
			KswReq *r = reqs[ri];
			wmo_ez_t ez;
			std::vector<uint8_t> q(r->ql > 0 ? r->ql : 0), t(r->tl > 0 ? r->tl : 0);
			r->copy_query(q.data()); r->copy_target(t.data());
			check_positions(*r, q, t);
			std::vector<uint32_t> cig(q.size() + t.size() + 4);
			wmo_ksw_exts2((int)q.size(), q.data(), (int)t.size(), t.data(), 5, mat, sc.q, sc.e, sc.q2, noncan, r->zdrop, junc_bonus, r->flag, r->junc.empty() ? 0 : r->junc.data(), &ez, cig.data());
			r->ez.max = ez.max; r->ez.zdropped = ez.zdropped; r->ez.max_q = ez.max_q; r->ez.max_t = ez.max_t; r->ez.mqe = ez.mqe; r->ez.mqe_t = ez.mqe_t;
			r->ez.mte = ez.mte; r->ez.mte_q = ez.mte_q; r->ez.score = ez.score; r->ez.reach_end = ez.reach_end; r->ez.n_cigar = ez.n_cigar; r->ez.cig_off = 0;
			r->cigar.assign(cig.begin(), cig.begin() + ez.n_cigar);
		});
	}
};

struct Harness { Index idx; wmo_bloom_t *bloom; };
static std::atomic<long> g_pos_checked{0}, g_pos_bad{0};       // resident-position checks of all OracleOps so far (h_pos_check)
static void note_pos(const OracleOps &o) { g_pos_checked += o.n_pos_checked.load(); g_pos_bad += o.n_pos_bad.load(); }

extern "C" {

void *h_index_build_flag(const char *fasta, const char *kmer_file, int k, int w, int idx_flag, int n_threads);
void *h_index_build(const char *fasta, const char *kmer_file, int k, int w, int n_threads) { return h_index_build_flag(fasta, kmer_file, k, w, 0, n_threads); }
void *h_index_build_flag(const char *fasta, const char *kmer_file, int k, int w, int idx_flag, int n_threads)      // idx_flag 1 = MM_I_HPC (-H)
{
	Harness *h = new Harness();
	IdxOpt io; io.k = k; io.w = w; io.flag = idx_flag;
	std::string err;
	if (index_build_from_fasta(io, fasta, kmer_file ? kmer_file : "", n_threads, h->idx, err) < 0) { fprintf(stderr, "h_index_build: %s\n", err.c_str()); delete h; return 0; }
	std::vector<uint64_t> kms;
	if (kmer_file && kmer_file[0]) { std::ifstream in(kmer_file); std::string km; uint64_t f; while (in >> km >> f) kms.push_back(wmo_encode_kmer(km.c_str(), (int)km.size())); }
	h->bloom = wmo_bloom_new(kms.size());
	for (uint64_t x : kms) wmo_bloom_insert(h->bloom, x);
	return h;
}
int h_index_read_bed(void *hv, const char *path) { std::string err; return index_read_bed(((Harness*)hv)->idx, path, true, err); }      // --junc-bed
int h_bed_junc(void *hv, int ctg, int st, int en, uint8_t *out) { return ((Harness*)hv)->idx.bed_junc(ctg, st, en, out); }
int h_getseq(void *hv, uint32_t rid, uint32_t st, uint32_t en, uint8_t *out) { return ((Harness*)hv)->idx.getseq(rid, st, en, out); }
uint64_t h_index_n_minimizers(void *hv) { return ((Harness*)hv)->idx.n_minimizers; }
int h_index_get(void *hv, uint64_t minier, uint64_t *out, int cap)
{
	int n; const uint64_t *p = ((Harness*)hv)->idx.get(minier, &n);
	for (int i = 0; i < n && i < cap; ++i) out[i] = p[i];
	return n;
}
int64_t h_sketch(void *hv, const char *seq, int len, int w, int k, uint32_t rid, uint64_t *ox, uint64_t *oy, int64_t cap)
{
	std::vector<m128> v;
	sketch(seq, len, w, k, rid, &((Harness*)hv)->idx.bloom, v, (((Harness*)hv)->idx.flag & 1) != 0);
	for (size_t i = 0; i < v.size() && (int64_t)i < cap; ++i) ox[i] = v[i].x, oy[i] = v[i].y;
	return (int64_t)v.size();
}
void h_radix_sort_128x(uint64_t *x, uint64_t *y, int64_t n)
{
	std::vector<m128> a(n);
	for (int64_t i = 0; i < n; ++i) a[i].x = x[i], a[i].y = y[i];
	radix_sort_128x(a.data(), a.data() + n);
	for (int64_t i = 0; i < n; ++i) x[i] = a[i].x, y[i] = a[i].y;
}
void h_radix_sort_128x_parallel(uint64_t *x, uint64_t *y, int64_t n, int n_threads)
{
	std::vector<m128> a(n);
	for (int64_t i = 0; i < n; ++i) a[i].x = x[i], a[i].y = y[i];
	radix_sort_128x_parallel(a.data(), a.data() + n, n_threads);
	for (int64_t i = 0; i < n; ++i) x[i] = a[i].x, y[i] = a[i].y;
}
// parallel_tasks (wm_core.h): every index exactly once, on the plain path and through a ParHook with the coarse-task chunk hint
int h_parallel_tasks_selftest(int n_threads, int n)
{
	std::vector<std::atomic<int>> hit(n);
	for (auto &h : hit) h.store(0);
	parallel_tasks(n_threads, (size_t)n, [&](size_t i) { hit[i].fetch_add(1); });
	for (auto &h : hit) if (h.load() != 1) return -1;
	struct Hook : ParHook {
		size_t chunk_seen = 0;
		void run(size_t m, const std::function<void(size_t)> &fn) override { chunk_seen = tl_par_chunk(); tl_par_chunk() = 0; for (size_t i = 0; i < m; ++i) fn(i); }
	} hook;
	tl_par_hook() = &hook;
	parallel_tasks(n_threads, (size_t)n, [&](size_t i) { hit[i].fetch_add(1); });
	tl_par_hook() = 0;
	for (auto &h : hit) if (h.load() != 2) return -2;
	if (n >= 2 && hook.chunk_seen != 1) return -3;          // coarse tasks ask the hook for chunks of one
	return tl_par_chunk() == 0 ? 0 : -4;
}
// the vectorised host routines against their portable specifications (wm_align.cpp): ksw_ll_i16 and the scan of mm_update_extra
int h_extra_walk_both(const uint8_t *q, const uint8_t *t, const uint32_t *cigar, int n_cigar, int match, int mismatch, int ambi, int gq, int ge, int32_t *fast6, int32_t *generic6)
{
	wm::extra_walk_both(q, t, cigar, n_cigar, match, mismatch, ambi, gq, ge, fast6, generic6);
	return 0;
}
int h_ll_i16_portable(int qlen, const uint8_t *q, int tlen, const uint8_t *t, const int8_t *mat, int gapo, int gape, int *qe, int *te)
{
#if defined(__SSE2__)
	return ll_i16_portable(qlen, q, tlen, t, mat, gapo, gape, qe, te);
#else
	return ll_i16(qlen, q, tlen, t, mat, gapo, gape, qe, te);
#endif
}
int h_ll_i16(int qlen, const uint8_t *q, int tlen, const uint8_t *t, const int8_t *mat, int gapo, int gape, int *qe, int *te) { return ll_i16(qlen, q, tlen, t, mat, gapo, gape, qe, te); }

int64_t h_chain_extract(int64_t n, const uint64_t *ax, const uint64_t *ay, const int32_t *f, const int32_t *p, const int32_t *v, int min_cnt, int min_sc,
                        int *n_u, uint64_t *u_out, uint64_t *bx, uint64_t *by)
{
	std::vector<m128> a(n);
	for (int64_t i = 0; i < n; ++i) a[i].x = ax[i], a[i].y = ay[i];
	std::vector<uint64_t> u; std::vector<m128> b;
	chain_extract(n, a.data(), f, p, v, min_cnt, min_sc, u, b);
	*n_u = (int)u.size();
	for (size_t i = 0; i < u.size(); ++i) u_out[i] = u[i];
	for (size_t i = 0; i < b.size(); ++i) bx[i] = b[i].x, by[i] = b[i].y;
	return (int64_t)b.size();
}
float h_avg_qspan(int64_t n, const uint64_t *ay) { std::vector<m128> a(n); for (int64_t i = 0; i < n; ++i) a[i].y = ay[i]; return chain_avg_qspan(n, a.data()); }
void h_index_view(void *hv, const uint64_t **hkey, const uint64_t **hval, const uint64_t **P, int *hbits, uint64_t *nslots, uint64_t *np)
{
	Index &ix = ((Harness*)hv)->idx;
	*hkey = ix.hkey.data(); *hval = ix.hval.data(); *P = ix.P.data(); *hbits = ix.hbits; *nslots = ix.hkey.size(); *np = ix.P.size();
}
void h_bloom_view(void *hv, uint32_t *table_bits, uint32_t *salts, const uint8_t **bits)
{
	Index &ix = ((Harness*)hv)->idx;
	*table_bits = (uint32_t)ix.bloom.table_bits; salts[0] = ix.bloom.salt[0]; salts[1] = ix.bloom.salt[1]; *bits = ix.bloom.bits.data();
}

// index files in the reference's format
int h_index_save_mmi(void *hv, const char *path) { std::string err; return index_save_mmi(((Harness*)hv)->idx, path, err); }
void *h_index_load_mmi(const char *path, const char *kmer_file)
{
	Harness *h = new Harness();
	std::string err;
	if (index_load_mmi(path, kmer_file ? kmer_file : "", h->idx, err) < 0) { fprintf(stderr, "%s\n", err.c_str()); delete h; return 0; }
	std::vector<uint64_t> kms;                                        // the oracle-backed sketch op uses the oracle's own filter
	if (kmer_file && kmer_file[0]) { std::ifstream in(kmer_file); std::string km; uint64_t f; while (in >> km >> f) kms.push_back(wmo_encode_kmer(km.c_str(), (int)km.size())); }
	h->bloom = wmo_bloom_new(kms.size());
	for (uint64_t x : kms) wmo_bloom_insert(h->bloom, x);
	return h;
}

// same output layout as refshim_map (oracle/ref_shim.cpp)
static int64_t g_max_sw_mat = 0, g_flag_clear = 0;
static thread_local int g_last_rl_defined = 1;
int h_last_rep_len_defined() { return g_last_rl_defined; }        // of the last h_map call on this thread: did the mapper ASSIGN rep_len where the reference does (src/map.c:808-813, 859-861)
void h_set_flag_clear(int64_t bits) { g_flag_clear = bits; }     // option bits the h_map* calls that follow clear after the preset (e.g. -uf clears MM_F_SPLICE_REV)
int h_map(void *hv, const char *preset, int64_t flag_extra, const char *seq, int len, const char *name,
          int32_t *hit_out, int hit_cap, uint32_t *cig_out, int64_t cig_cap, int64_t *n_cig_total, uint64_t *stats_out)
{
	Harness *h = (Harness*)hv;
	IdxOpt io; MapOpt mo;
	set_preset(0, io, mo);
	if (preset && preset[0] && set_preset(preset, io, mo) < 0) return -1;
	mo.flag |= flag_extra; mo.flag &= ~g_flag_clear;
	mapopt_update(mo, h->idx);
	OracleOps ops; ops.idx = &h->idx; ops.bloom = h->bloom; ops.opt = &mo;
	std::vector<ReadIn> reads(1);
	reads[0].name = name; reads[0].seq.assign(seq, len);
	std::vector<ReadOut> out;
	MapStats st;
	map_batch(h->idx, mo, &ops, reads, out, &st);
	note_pos(ops);
	if (!st.internal_error.empty()) { fprintf(stderr, "[harness] %s\n", st.internal_error.c_str()); return -5; }      // a violated invariant of the host mapper (it used to be dropped here)
	if (ops.n_pos_bad.load()) return -3;
	if (stats_out) { stats_out[0] = st.n_flush; stats_out[1] = st.n_ksw; stats_out[2] = st.n_chain; stats_out[3] = st.n_sketch; }
	int64_t nc = 0;
	const std::vector<Reg> &regs = out[0].regs;
	g_last_rl_defined = out[0].rep_len_defined ? 1 : 0;
	for (size_t i = 0; i < regs.size() && (int)i < hit_cap; ++i) {
		const Reg &r = regs[i];
		int32_t *o = hit_out + 16 * i;
		o[0] = r.rid; o[1] = r.rs; o[2] = r.re; o[3] = r.qs; o[4] = r.qe; o[5] = r.rev; o[6] = r.mapq; o[7] = r.has_p ? (int)r.cigar.size() : 0;
		o[8] = r.score; o[9] = r.cnt; o[10] = r.mlen; o[11] = r.blen; o[12] = r.dp_score; o[13] = r.dp_max; o[14] = r.dp_max2;
		o[15] = (r.parent == r.id) | r.inv << 1 | r.sam_pri << 2 | r.split << 3 | (r.has_p ? r.trans_strand << 5 : 0);
		for (uint32_t c : r.cigar) { if (nc < cig_cap) cig_out[nc] = c; ++nc; }
	}
	*n_cig_total = nc;
	return (int)regs.size();
}

// how many requests carried resident positions (checked against their host views) and how many of them disagreed
void h_pos_check(long *checked, long *bad) { *checked = g_pos_checked.load(); *bad = g_pos_bad.load(); }

void h_set_max_sw_mat(int64_t v) { g_max_sw_mat = v; }          // mm_mapopt_t::max_sw_mat for the h_map_many calls that follow (src/align.c:323-325)

// several reads at once on a team of `n_threads` schedulers; hits of read i start at hit_first[i] (16 ints each)
int h_map_many(void *hv, const char *preset, int64_t flag_extra, int n, const char *const *seqs, const int *lens, int n_threads,
               int32_t *hit_out, int hit_cap, int64_t *hit_first, uint32_t *cig_out, int64_t cig_cap, int64_t *n_cig_total)
{
	Harness *h = (Harness*)hv;
	IdxOpt io; MapOpt mo;
	set_preset(0, io, mo);
	if (preset && preset[0] && set_preset(preset, io, mo) < 0) return -1;
	mo.flag |= flag_extra; mo.flag &= ~g_flag_clear;
	mo.max_sw_mat = g_max_sw_mat;
	mapopt_update(mo, h->idx);
	OracleOps ops; ops.idx = &h->idx; ops.bloom = h->bloom; ops.opt = &mo;
	std::vector<ReadIn> reads(n);
	for (int i = 0; i < n; ++i) { reads[i].name = "read" + std::to_string(i); reads[i].seq.assign(seqs[i], lens[i]); }
	std::vector<ReadOut> out;
	map_batch(h->idx, mo, &ops, reads, out, 0, n_threads);
	note_pos(ops);
	if (ops.n_pos_bad.load()) return -3;
	if (prof_on()) prof_report(stderr);
	int64_t nc = 0; int nh = 0;
	for (int k = 0; k < n; ++k) {
		hit_first[k] = nh;
		for (const Reg &r : out[k].regs) {
			if (nh >= hit_cap) return -2;
			int32_t *o = hit_out + 16 * (size_t)nh++;
			o[0] = r.rid; o[1] = r.rs; o[2] = r.re; o[3] = r.qs; o[4] = r.qe; o[5] = r.rev; o[6] = r.mapq; o[7] = r.has_p ? (int)r.cigar.size() : 0;
			o[8] = r.score; o[9] = r.cnt; o[10] = r.mlen; o[11] = r.blen; o[12] = r.dp_score; o[13] = r.dp_max; o[14] = r.dp_max2;
			o[15] = (r.parent == r.id) | r.inv << 1 | r.sam_pri << 2 | r.split << 3 | (r.has_p ? r.trans_strand << 5 : 0);
			for (uint32_t c : r.cigar) { if (nc < cig_cap) cig_out[nc] = c; ++nc; }
		}
	}
	hit_first[n] = nh;
	*n_cig_total = nc;
	return nh;
}

// formatted records (PAF, or SAM with MM_F_OUT_SAM in flag_extra) of several reads; returns the text length (or -needed)
int64_t h_map_text(void *hv, const char *preset, int64_t flag_extra, int n, const char *const *names, const char *const *seqs, const int *lens, int n_threads,
                   char *out, int64_t cap)
{
	Harness *h = (Harness*)hv;
	IdxOpt io; MapOpt mo;
	set_preset(0, io, mo);
	if (preset && preset[0] && set_preset(preset, io, mo) < 0) return -1;
	mo.flag |= flag_extra; mo.flag &= ~g_flag_clear;
	mapopt_update(mo, h->idx);
	OracleOps ops; ops.idx = &h->idx; ops.bloom = h->bloom; ops.opt = &mo;
	std::vector<ReadIn> reads(n);
	for (int i = 0; i < n; ++i) { reads[i].name = names[i]; reads[i].seq.assign(seqs[i], lens[i]); }
	std::vector<ReadOut> outv;
	map_batch(h->idx, mo, &ops, reads, outv, 0, n_threads);
	note_pos(ops);
	if (ops.n_pos_bad.load()) return -3;
	std::string text;
	for (int i = 0; i < n; ++i) write_read(text, h->idx, reads[i], outv[i], mo.flag);
	if ((int64_t)text.size() > cap) return -(int64_t)text.size();
	memcpy(out, text.data(), text.size());
	return (int64_t)text.size();
}

// the file-level pipeline (host/wm_pipeline.cpp) over oracle-backed ops: FASTA/FASTQ(.gz) -> PAF/SAM file
int h_map_file(void *hv, const char *preset, int64_t flag_extra, const char *reads_path, const char *out_path, int64_t mini_batch_bases, int n_threads, double *stats)
{
	Harness *h = (Harness*)hv;
	IdxOpt io; MapOpt mo;
	set_preset(0, io, mo);
	if (preset && preset[0] && set_preset(preset, io, mo) < 0) return -1;
	mo.flag |= flag_extra; mo.flag &= ~g_flag_clear;
	mapopt_update(mo, h->idx);
	OracleOps ops; ops.idx = &h->idx; ops.bloom = h->bloom; ops.opt = &mo;
	FILE *out = fopen(out_path, "wb");
	if (!out) return -2;
	std::string err;
	FileStats fs;
	const int rc = map_file(reads_path, mini_batch_bases, (mo.flag & 0x8) != 0, [&](std::vector<ReadIn> &batch, std::string &text, int lane) {
		std::vector<ReadOut> outv;
		map_batch(h->idx, mo, &ops, batch, outv, 0, n_threads, 0, lane);
		for (size_t i = 0; i < batch.size(); ++i) write_read(text, h->idx, batch[i], outv[i], mo.flag);
		return 0;
	}, out, &fs, err);
	fclose(out);
	if (stats) { stats[0] = (double)fs.n_reads; stats[1] = (double)fs.n_bases; stats[2] = (double)fs.n_batches; }
	return rc;
}

// a reference indexed in parts + the merge (host/wm_pipeline.cpp: map_file_split) over oracle-backed ops; returns the number of parts or < 0
int h_map_file_split(const char *fasta, const char *kmer_file, int k, int w, int64_t batch_bases, const char *preset, int64_t flag_extra,
                     const char *reads_path, const char *out_path, int64_t mini_batch_bases, int n_threads)
{
	IdxOpt io; MapOpt mo;
	set_preset(0, io, mo);
	if (preset && preset[0] && set_preset(preset, io, mo) < 0) return -1;
	io.k = k; io.w = w;
	mo.flag |= flag_extra; mo.flag &= ~g_flag_clear;
	std::string err;
	std::vector<uint64_t> kms;
	if (kmer_file && kmer_file[0]) { std::ifstream in(kmer_file); std::string km; uint64_t f; while (in >> km >> f) kms.push_back(wmo_encode_kmer(km.c_str(), (int)km.size())); }
	wmo_bloom_t *bloom = wmo_bloom_new(kms.size());
	for (uint64_t x : kms) wmo_bloom_insert(bloom, x);
	// one part at a time (src/main.c:398-429): the next part is read and built when its turn comes, mapped, spilled and destroyed
	IndexPartReader rd;
	if (rd.open(fasta, err) < 0) { fprintf(stderr, "h_map_file_split: %s\n", err.c_str()); return -2; }
	SplitRun run(reads_path, mini_batch_bases, mo, k, w);
	std::vector<std::string> names, seqs;
	std::vector<size_t> part_seqs;
	int n_parts = 0;
	while (rd.next((uint64_t)batch_bases, names, seqs) > 0) {
		Index part;
		if (index_build(io, names, seqs, kmer_file ? kmer_file : "", n_threads, part, err) < 0) { fprintf(stderr, "h_map_file_split: %s\n", err.c_str()); return -2; }
		std::vector<std::string>().swap(seqs);
		MapOpt cur = mo;
		mapopt_update(cur, part);
		OracleOps ops; ops.idx = &part; ops.bloom = bloom; ops.opt = &cur;
		const int rc = run.add_part(part.seq, [&](std::vector<ReadIn> &batch, std::vector<ReadOut> &o, int lane) -> int { map_batch(part, cur, &ops, batch, o, 0, n_threads, 0, lane); return 0; }, err);
		if (rc) { fprintf(stderr, "h_map_file_split: %s\n", err.c_str()); return -4; }
		part_seqs.push_back(part.seq.size());
		++n_parts;
	}
	{   // the parts formed one at a time are the parts the all-at-once builder forms
		std::vector<Index> all;
		const int n2 = index_build_parts_from_fasta(io, fasta, kmer_file ? kmer_file : "", n_threads, (uint64_t)batch_bases, all, err);
		if (n2 != n_parts) { fprintf(stderr, "h_map_file_split: %d parts one at a time, %d at once\n", n_parts, n2); return -5; }
		for (int j = 0; j < n2; ++j) if (all[j].seq.size() != part_seqs[j]) { fprintf(stderr, "h_map_file_split: part %d differs\n", j); return -5; }
	}
	FILE *out = fopen(out_path, "wb");
	if (!out) return -3;
	if (mo.flag & 0x8) { std::string hdr; write_sam_header(hdr, run.dict(), 0, 0); fwrite(hdr.data(), 1, hdr.size(), out); }
	FileStats fs;
	const int rc = run.finish(out, &fs, err);
	fclose(out);
	if (rc) { fprintf(stderr, "h_map_file_split: %s\n", err.c_str()); return -4; }
	return n_parts;
}

// the mapper's own mm_test_zdrop (scan + verdict incl. the inversion test) and mm_update_extra (mm_fix_cigar + the vector scan), for
// tests/test_walks_vs_ref.py: compared with the reference's static functions (oracle/ref_align_shim.cpp)
int h_test_zdrop(int64_t flag, int zdrop, int zdrop_inv, int q, int e, int max_gap, int min_chain_score, int a, int min_dp_max,
                 const uint8_t *qseq, const uint8_t *tseq, const uint32_t *cigar, int n_cigar, const int8_t *mat)
{
	MapOpt o;
	o.flag = flag; o.zdrop = zdrop; o.zdrop_inv = zdrop_inv; o.q = q; o.e = e; o.max_gap = max_gap; o.min_chain_score = min_chain_score; o.a = a; o.min_dp_max = min_dp_max;
	std::vector<uint32_t> cg(cigar, cigar + n_cigar);
	return test_zdrop(o, qseq, tseq, cg, mat);
}
int h_update_extra(int rev, int qs, int qe, int rs, int re, const uint8_t *qseq, const uint8_t *tseq, const int8_t *mat, int q, int e,
                   const uint32_t *cigar, int n_cigar, int32_t *out6, uint32_t *cigar_out, int cap, int *n_out)
{
	Reg r;
	r.rev = rev; r.qs = qs; r.qe = qe; r.rs = rs; r.re = re; r.has_p = true;
	r.cigar.assign(cigar, cigar + n_cigar);
	update_extra(r, qseq, tseq, mat, q, e);
	out6[0] = r.blen; out6[1] = r.mlen; out6[2] = (int32_t)r.n_ambi; out6[3] = r.dp_max; out6[4] = rev ? r.qe : r.qs; out6[5] = r.rs;
	*n_out = (int)r.cigar.size();
	for (size_t i = 0; i < r.cigar.size() && (int)i < cap; ++i) cigar_out[i] = r.cigar[i];
	std::string ie;
	return take_internal_error(ie) ? -5 : 0;
}

int h_usable_cores(void) { return usable_cores(); }
// the product's host packer of the resident reads (csrc/reads2bit.h)
void h_pack_codes(const uint8_t *codes, size_t n, uint64_t *pk, uint64_t *nm) { wm_pack_codes(codes, n, pk, nm); }
size_t h_pk_words(size_t n) { return wm_pk_words(n); }
size_t h_nm_words(size_t n) { return wm_nm_words(n); }

// the host's compile of the CIGAR walks the device also runs (winnowmap_amd/csrc/cigar_walk.h)
void h_zdrop_walk(const uint8_t *q, const uint8_t *t, const uint32_t *cigar, int n_cigar, int match, int mismatch, int ambi, int gq, int ge, int32_t *out5)
{
	wm_zd_t z;
	wm_zdrop_walk(q, t, cigar, n_cigar, match, mismatch, ambi, gq, ge, &z);
	out5[0] = z.max_zdrop; out5[1] = z.t0; out5[2] = z.t1; out5[3] = z.q0; out5[4] = z.q1;
}
} // extern "C"

// ---- the batching hub on its own (host/wm_fiber.h): fibers that file one request of every kind against ops that only record what they are handed ----
namespace {
enum { HK_SKETCH, HK_SEED, HK_CHAIN, HK_WINDOW, HK_KSW, HK_EXTS2, HK_EXTRA, HK_FIX, HK_EQX, HK_CS, HK_N };
struct HubFakeOps : DeviceOps {
	std::mutex mu;
	std::set<const void*> got[HK_N];       // every request pointer a batch call of that kind was handed
	long dup = 0, bad_sc = 0;              // pointers handed over twice; final-pass calls that did not carry their requests' score
	std::atomic<int> chain_throws{0};      // the next so many chain_batch calls throw before they serve anything
	int max_inflight() const override { return 4; }
	template <class R> void note(int kind, const std::vector<R*> &reqs) { std::lock_guard<std::mutex> lk(mu); for (R *r : reqs) if (!got[kind].insert(r).second) ++dup; }
	void sketch_batch(int, int, std::vector<SketchReq*> &reqs) override { note(HK_SKETCH, reqs); for (SketchReq *r : reqs) r->mini.push_back(m128()); }
	void seed_batch(std::vector<SeedReq*> &reqs) override { note(HK_SEED, reqs); for (SeedReq *r : reqs) r->rep_len = 1; }
	void chain_batch(std::vector<ChainReq*> &reqs) override
	{
		note(HK_CHAIN, reqs);
		if (chain_throws.load() > 0 && chain_throws.fetch_sub(1) > 0) throw std::runtime_error("hub selftest: chain_batch throws");
		for (ChainReq *r : reqs) r->u.push_back(1);
	}
	void window_batch(int, int, std::vector<WindowReq*> &reqs) override { note(HK_WINDOW, reqs); for (WindowReq *r : reqs) r->n_anchors = 1; }
	void ksw_batch(const wm_ksw_score_t &, std::vector<KswReq*> &reqs) override { note(HK_KSW, reqs); for (KswReq *r : reqs) r->ez.score = 1; }
	void exts2_batch(const wm_ksw_score_t &, int, int, std::vector<KswReq*> &reqs) override { note(HK_EXTS2, reqs); for (KswReq *r : reqs) r->ez.score = 1; }
	void extra_batch(const wm_extra_score_t &sc, std::vector<ExtraReq*> &reqs) override { note(HK_EXTRA, reqs); if (sc.match != 7) ++bad_sc; for (ExtraReq *r : reqs) r->out.blen = 1; }
	void fix_extra_batch(const wm_extra_score_t &sc, std::vector<FixReq*> &reqs) override { note(HK_FIX, reqs); if (sc.match != 7) ++bad_sc; for (FixReq *r : reqs) r->qshift = 1; }
	void eqx_batch(std::vector<EqxReq*> &reqs) override { note(HK_EQX, reqs); for (EqxReq *r : reqs) r->in_place = true; }
	void cs_batch(std::vector<CsReq*> &reqs) override { note(HK_CS, reqs); for (CsReq *r : reqs) r->body->assign("x"); }
};
// everything one fiber files; it outlives the run, so that a request's address names it for good
struct HubFiberReqs {
	SketchReq sk; SeedReq sd; ChainReq ch; WindowReq wn;
	std::vector<KswReq> ks, ks_capped, ks_none;             // normal + heavy + huge + over max_sw_mat; only one over max_sw_mat; nothing
	std::vector<ExtraReq> ex, ex_none, fx_ex, only_ex;      // extra(); extra() of nothing; the extras beside fixes; the extras of fix_extra() without fixes
	std::vector<FixReq> fx, fx_alone, fx_none;              // with extras; without; nothing
	std::vector<EqxReq> eq; std::vector<CsReq> cs; std::string body[2];
	HubFiberReqs() : ks(4), ks_capped(1), ex(2), fx_ex(1), only_ex(1), fx(2), fx_alone(1), eq(2), cs(2)
	{
		const int len[4] = { 100, 3000, 40000, 50000 }, w[4] = { 10, 100, 500, 500 };      // ksw_units 400, 12000, 400000 (the default thresholds: 8192 and 131072); 2.5e9 cells
		for (int i = 0; i < 4; ++i) { ks[i].ql = ks[i].tl = len[i]; ks[i].w = w[i]; ks[i].cigar.assign(3, 1u); }
		ks_capped[0].ql = ks_capped[0].tl = 50000; ks_capped[0].cigar.assign(3, 1u);
		for (std::vector<ExtraReq> *v : { &ex, &fx_ex, &only_ex }) for (ExtraReq &r : *v) r.sc.match = 7;
		for (std::vector<FixReq> *v : { &fx, &fx_alone }) for (FixReq &r : *v) r.sc.match = 7;
		for (int i = 0; i < 2; ++i) cs[i].body = &body[i];
	}
};
// the four scheduling knobs of one operation as a fresh hub holds them
static void hub_knobs(const Hub &H, int op, double out[4])
{
	const OpKnobs &k = H.knob[op];
	out[0] = (double)k.min_more; out[1] = (double)k.max_op; out[2] = (double)k.min_batch; out[3] = k.max_wait_ms;
}
}

#define HUB_CHECK(c) do { if (!(c)) { fprintf(stderr, "[harness] hub selftest: %s fails (line %d)\n", #c, __LINE__); return -__LINE__; } } while (0)
#define HUB_FIBER_CHECK(c) do { if (!(c)) { int z = 0; if (fiber_fail.compare_exchange_strong(z, __LINE__)) fprintf(stderr, "[harness] hub selftest, in a fiber: %s fails (line %d)\n", #c, __LINE__); } } while (0)
extern "C" int wmh_hub_selftest(int n_threads, int n_fibers, int splice)
{
	const wm_ksw_score_t sc = {};
	// the scheduling table: the defaults, and every operation's four environment variables
	static const char *const stem[OP_N] = { "SKETCH", "SEED", "CHAIN", "KSW", "KSWH", "KSWX", "WINDOW", "WINDOWB", "EXTRA", "FIX", "EQX", "CS" };
	static const double dflt[OP_N][4] = {      // min_more, max_op, min_batch, max_wait_ms
		{ 4096, 2, 8192, 15 }, { 4096, 2, 8192, 15 }, { 4096, 2, 8192, 15 }, { 24576, 3, 98304, 30 }, { 2048, 2, 12288, 60 }, { 64, 1, 512, 250 },
		{ 4096, 3, 8192, 15 }, { 1024, 2, 2048, 30 }, { 8192, 2, 4096, 15 }, { 8192, 2, 4096, 15 }, { 8192, 2, 4096, 15 }, { 8192, 2, 4096, 15 } };
	static const char *const knob[4] = { "MIN_MORE", "MAX", "MIN_BATCH", "MAX_WAIT_MS" };
	static const char *const set_to[4] = { "11", "5", "13", "2.5" };
	static const double set_val[4] = { 11, 5, 13, 2.5 };
	{
		HubFakeOps ops;
		Hub H(&ops, sc, 50, 15);
		HUB_CHECK(H.max_inflight == 4);
		for (int op = 0; op < OP_N; ++op) { double k[4]; hub_knobs(H, op, k); for (int j = 0; j < 4; ++j) HUB_CHECK(k[j] == dflt[op][j]); }
		for (int op = 0; op < OP_N; ++op) {
			char key[64];
			for (int j = 0; j < 4; ++j) { snprintf(key, sizeof(key), "WM_%s_%s", stem[op], knob[j]); setenv(key, set_to[j], 1); }
			Hub E(&ops, sc, 50, 15);
			for (int j = 0; j < 4; ++j) { snprintf(key, sizeof(key), "WM_%s_%s", stem[op], knob[j]); unsetenv(key); }
			for (int o = 0; o < OP_N; ++o) { double k[4]; hub_knobs(E, o, k); for (int j = 0; j < 4; ++j) HUB_CHECK(k[j] == (o == op ? set_val[j] : dflt[o][j])); }
		}
	}
	const int T = n_threads < 1 ? 1 : n_threads;
	std::atomic<int> fiber_fail{0}, finished{0};
	auto run_team = [&](Hub &hub, ErrorSink &sink, const std::function<void(Scheduler&, int)> &body, int n) {
		hub.n_workers = T;
		std::vector<std::unique_ptr<Scheduler>> sch(T);
		for (int t = 0; t < T; ++t) { sch[t].reset(new Scheduler(&hub, t)); sch[t]->hold((n - t + T - 1) / T); }      // (as map_batch: nobody sees the call finished before every worker has spawned its fibers)
		auto work = [&](int t) {
			ErrorSink *const prev = tl_error_sink();
			tl_error_sink() = &sink;
			for (int i = t; i < n; i += T) { Scheduler *s = sch[t].get(); s->spawn([&body, s, i]() { body(*s, i); }); s->release(1); }
			sch[t]->run();
			tl_error_sink() = prev;
		};
		std::vector<std::thread> th;
		for (int t = 1; t < T; ++t) th.emplace_back(work, t);
		work(0);
		for (auto &x : th) x.join();
	};
	{   // every filing call once per fiber
		HubFakeOps ops;
		Hub hub(&ops, sc, 50, 15);
		hub.splice = splice != 0;
		hub.max_sw_mat = 2000000000;
		std::vector<std::unique_ptr<HubFiberReqs>> reqs(n_fibers);
		for (auto &r : reqs) r.reset(new HubFiberReqs());
		ErrorSink sink;
		run_team(hub, sink, [&](Scheduler &s, int i) {
			HubFiberReqs &r = *reqs[i];
			s.sketch(r.sk); HUB_FIBER_CHECK(r.sk.mini.size() == 1);
			s.seed(r.sd); HUB_FIBER_CHECK(r.sd.rep_len == 1);
			s.chain(r.ch); HUB_FIBER_CHECK(r.ch.u.size() == 1);
			s.window(r.wn); HUB_FIBER_CHECK(r.wn.n_anchors == 1);
			s.ksw(r.ks);                                            // three queues (one under splice), one wait; the fourth request is over --cap-sw-mat
			for (int j = 0; j < 3; ++j) HUB_FIBER_CHECK(r.ks[j].ez.score == 1 && r.ks[j].cigar.size() == 3);
			s.ksw(r.ks_capped); s.ksw(r.ks_none);                   // nothing to wait for
			for (const KswReq *c : { &r.ks[3], &r.ks_capped[0] }) HUB_FIBER_CHECK(c->ez.zdropped == 1 && c->ez.score == -0x40000000 && c->cigar.empty());
			s.extra(r.ex); s.extra(r.ex_none);
			for (ExtraReq &e : r.ex) HUB_FIBER_CHECK(e.out.blen == 1);
			s.fix_extra(r.fx, r.fx_ex);                             // both lists: one wait for two operations
			for (FixReq &f : r.fx) HUB_FIBER_CHECK(f.qshift == 1);
			HUB_FIBER_CHECK(r.fx_ex[0].out.blen == 1);
			s.fix_extra(r.fx_none, r.only_ex); HUB_FIBER_CHECK(r.only_ex[0].out.blen == 1);
			s.fix_extra(r.fx_alone, r.ex_none); HUB_FIBER_CHECK(r.fx_alone[0].qshift == 1);
			s.fix_extra(r.fx_none, r.ex_none);                      // returns at once
			s.eqx(r.eq); for (EqxReq &e : r.eq) HUB_FIBER_CHECK(e.in_place);
			s.cs(r.cs); for (int j = 0; j < 2; ++j) HUB_FIBER_CHECK(r.body[j] == "x");
			++finished;
		}, n_fibers);
		HUB_CHECK(fiber_fail.load() == 0);
		HUB_CHECK(finished.load() == n_fibers);
		HUB_CHECK(sink.msg.empty());
		HUB_CHECK(ops.dup == 0 && ops.bad_sc == 0);
		std::set<const void*> want[HK_N];
		for (auto &p : reqs) {
			HubFiberReqs &r = *p;
			want[HK_SKETCH].insert(&r.sk); want[HK_SEED].insert(&r.sd); want[HK_CHAIN].insert(&r.ch); want[HK_WINDOW].insert(&r.wn);
			for (int j = 0; j < 3; ++j) want[splice ? HK_EXTS2 : HK_KSW].insert(&r.ks[j]);
			for (std::vector<ExtraReq> *v : { &r.ex, &r.fx_ex, &r.only_ex }) for (ExtraReq &e : *v) want[HK_EXTRA].insert(&e);
			for (std::vector<FixReq> *v : { &r.fx, &r.fx_alone }) for (FixReq &f : *v) want[HK_FIX].insert(&f);
			for (EqxReq &e : r.eq) want[HK_EQX].insert(&e);
			for (CsReq &c : r.cs) want[HK_CS].insert(&c);
		}
		for (int k = 0; k < HK_N; ++k) HUB_CHECK(ops.got[k] == want[k]);
		const uint64_t n = (uint64_t)n_fibers;
		const uint64_t filed[OP_N] = { n, n, n, splice ? 3 * n : n, splice ? 0 : n, splice ? 0 : n, n, 0, 4 * n, 3 * n, 2 * n, 2 * n };
		for (int op = 0; op < OP_N; ++op) { HUB_CHECK(hub.n_reqs[op] == filed[op]); HUB_CHECK(filed[op] ? hub.n_batches[op] >= 1 : hub.n_batches[op] == 0); }
	}
	{   // a batch call that throws: its waiters resume (their requests unserved), the call's sink has the message, later batches run
		HubFakeOps ops;
		ops.chain_throws = 1;
		Hub hub(&ops, sc, 50, 15);
		std::vector<ChainReq> first(n_fibers), second(n_fibers);
		ErrorSink sink;
		finished = 0;
		run_team(hub, sink, [&](Scheduler &s, int i) { s.chain(first[i]); s.chain(second[i]); ++finished; }, n_fibers);
		HUB_CHECK(finished.load() == n_fibers);
		HUB_CHECK(sink.msg.find("chain_batch throws") != std::string::npos);
		HUB_CHECK(ops.dup == 0 && ops.got[HK_CHAIN].size() == 2 * (size_t)n_fibers);
		HUB_CHECK(hub.n_reqs[OP_CHAIN] == 2 * (uint64_t)n_fibers && hub.n_batches[OP_CHAIN] >= 2);
		size_t served = 0;
		for (int i = 0; i < n_fibers; ++i) served += first[i].u.size() + second[i].u.size();
		HUB_CHECK(served >= 1 && served < 2 * (size_t)n_fibers);      // (the batch that threw served nobody; every other batch served its requests)
	}
	return 0;
}

// ---- the batch planner of the final-CIGAR device calls on its own (host/wm_final_plan.h): every expectation below is a literal table ----
namespace {
int fp_code = 0, fp_calls = 0;
char fp_msg[512] = "";
int fp_err(int code, const char *fmt, ...)         // set_err's signature: records instead
{
	va_list ap;
	va_start(ap, fmt);
	vsnprintf(fp_msg, sizeof(fp_msg), fmt, ap);
	va_end(ap);
	fp_code = code; ++fp_calls;
	return code;
}
int fp_measured = 0;                               // calls of the measure below
int fp_measure(int, const uint32_t *cig, int nc, int64_t *qlen, int64_t *tlen, int64_t *cols)      // M / I / D lengths, nothing refused
{
	++fp_measured;
	for (int k = 0; k < nc; ++k) {
		const uint32_t op = cig[k] & 0xf, len = cig[k] >> 4;
		if (op == 0) { *qlen += len; *tlen += len; *cols += len; }
		else if (op == 1) { *qlen += len; *cols += len; }
		else if (op == 2) { *tlen += len; *cols += len; }
	}
	return 0;
}
bool fp_pairs(const std::vector<wm_final_pair> &v, std::initializer_list<std::pair<int, int>> want)
{
	if (v.size() != want.size()) return false;
	size_t i = 0;
	for (const auto &w : want) { if (v[i].x != w.first || v[i].y != w.second) return false; ++i; }
	return true;
}
bool fp_zero(const wm_extra_djob_t &d) { static const wm_extra_djob_t z = {}; return memcmp(&d, &z, sizeof(d)) == 0; }
constexpr uint32_t fp_M(uint32_t len) { return len << 4; }
constexpr uint32_t fp_I(uint32_t len) { return len << 4 | 1; }
constexpr uint32_t fp_D(uint32_t len) { return len << 4 | 2; }
}

#define FP_CHECK(c) do { if (!(c)) { fprintf(stderr, "[harness] final plan selftest: %s fails (line %d; last message \"%s\")\n", #c, __LINE__, fp_msg); return -__LINE__; } } while (0)
extern "C" int wmh_final_plan_selftest(void)
{
	const int LMIN = 128, TILE = 64;
	const uint32_t seq_len[2] = { 500, 300 };
	const uint64_t seq_off[2] = { 0, 512 };
	const FinalView view = { 1000, seq_len, seq_off, 2 };
	FinalPlan plan;
	fp_calls = 0; fp_msg[0] = 0;
	{   // routing: columns 0 (empty CIGAR), 127, 128, 129, 64
		const uint32_t cig[5] = { fp_M(127), fp_M(100), fp_I(28), fp_M(129), fp_M(64) };
		const wm_extra_job_t jobs[5] = { { 0, 0, 0, 0 }, { 0, 0, 0, 1 }, { 0, 0, 1, 2 }, { 0, 0, 3, 1 }, { 0, 0, 4, 1 } };
		static const uint32_t pre_off[2][5] = { { 0, 1, 3, 6, 8 }, { 0, 2, 5, 9, 12 } };
		static const size_t n_pre[2] = { 10, 15 };
		static const int32_t tile0[5] = { 0, 0, 0, 2, 0 };
		for (int slack = 1; slack <= 2; ++slack) {
			FP_CHECK(final_plan(view, 5, jobs, 1000, 0, cig, 5, slack, LMIN, TILE, fp_err, fp_measure, plan) == WM_OK);
			FP_CHECK(plan.dj.size() == 5 && plan.order == (std::vector<int>{ 0, 1, 4 }));
			FP_CHECK(fp_pairs(plan.tmap, { { 2, 0 }, { 2, 1 }, { 3, 0 }, { 3, 1 }, { 3, 2 } }));
			FP_CHECK(fp_pairs(plan.lmap, { { 2, 2 }, { 3, 3 } }));
			for (int i = 0; i < 5; ++i) {
				const wm_extra_djob_t &d = plan.dj[i];
				FP_CHECK(d.tile0 == tile0[i] && d.pre_off == pre_off[slack - 1][i] && d.cig_off == jobs[i].cig_off && d.n_cigar == jobs[i].n_cigar);
				FP_CHECK(d.q_base == 0 && d.t_base == 0 && d.q_pos == 0 && d.q_len == 0);
			}
			FP_CHECK(plan.n_pre == n_pre[slack - 1]);
		}
		// long_min = 0: the empty job stays short, every other one is long
		static const int32_t tile0_all[5] = { 0, 0, 2, 4, 7 };
		FP_CHECK(final_plan(view, 5, jobs, 1000, 0, cig, 5, 1, 0, TILE, fp_err, fp_measure, plan) == WM_OK);
		FP_CHECK(plan.order == (std::vector<int>{ 0 }));
		FP_CHECK(fp_pairs(plan.tmap, { { 1, 0 }, { 1, 1 }, { 2, 0 }, { 2, 1 }, { 3, 0 }, { 3, 1 }, { 3, 2 }, { 4, 0 } }));
		FP_CHECK(fp_pairs(plan.lmap, { { 1, 2 }, { 2, 2 }, { 3, 3 }, { 4, 1 } }));
		for (int i = 0; i < 5; ++i) FP_CHECK(plan.dj[i].tile0 == tile0_all[i]);
		// two jobs on one CIGAR range: a prefix slot each
		const wm_extra_job_t twice[2] = { { 0, 0, 1, 2 }, { 0, 0, 1, 2 } };
		FP_CHECK(final_plan(view, 2, twice, 1000, 0, cig, 5, 1, LMIN, TILE, fp_err, fp_measure, plan) == WM_OK);
		FP_CHECK(plan.dj[0].pre_off == 0 && plan.dj[1].pre_off == 3 && plan.n_pre == 6 && plan.dj[0].cig_off == 1 && plan.dj[1].cig_off == 1);
		FP_CHECK(plan.dj[0].tile0 == 0 && plan.dj[1].tile0 == 2 && fp_pairs(plan.lmap, { { 0, 2 }, { 1, 2 } }));
		FP_CHECK(fp_calls == 0);
	}
	// operands: one CIGAR of 15 query and 13 target bases
	const uint32_t cig[3] = { fp_M(10), fp_I(5), fp_D(3) };
	const wm_extra_pos_t good = { 100, 50, 0, 0, 0, 0, 3 };
	{   // the accepted edges, position form
		const wm_extra_pos_t pos[5] = {
			{ 100, 50, -16, 0, 0, 0, 3 },            // q_pos == -16
			{ 100, 50, 101, 1, 7, 0, 3 },            // q_pos + qlen == 2 * qwin_len + 16
			{ 100, 50, 0, 1, 287, 0, 3 },            // t_pos + tlen == seq_len[rid]
			{ 950, 50, 0, 0, 0, 0, 3 },              // qwin_off + qwin_len == reads_bytes
			{ -5, -1, -1000, 99, -3, 3, 0 } };       // no CIGAR: the positions are not looked at
		static const long long q_base[5] = { 100, 100, 100, 950, 0 }, t_base[5] = { 0, 519, 799, 0, 0 };
		static const int32_t q_pos[5] = { -16, 101, 0, 0, 0 }, q_len[5] = { 50, 50, 50, 50, 0 };
		static const uint32_t pre_off[5] = { 0, 4, 8, 12, 16 };
		FP_CHECK(final_plan(view, 5, 0, 0, pos, cig, 3, 1, LMIN, TILE, fp_err, fp_measure, plan) == WM_OK);
		FP_CHECK(fp_calls == 0 && plan.order == (std::vector<int>{ 0, 1, 2, 3, 4 }) && plan.tmap.empty() && plan.lmap.empty() && plan.n_pre == 17);
		for (int i = 0; i < 5; ++i) {
			const wm_extra_djob_t &d = plan.dj[i];
			FP_CHECK(d.q_base == q_base[i] && d.t_base == t_base[i] && d.q_pos == q_pos[i] && d.q_len == q_len[i] && d.pre_off == pre_off[i] && d.tile0 == 0);
			FP_CHECK(d.cig_off == pos[i].cig_off && d.n_cigar == pos[i].n_cigar);
		}
		// ... and byte form: both operands end with seqs
		const wm_extra_job_t jobs[2] = { { 85, 0, 0, 3 }, { 0, 87, 0, 3 } };
		FP_CHECK(final_plan(view, 2, jobs, 100, 0, cig, 3, 1, LMIN, TILE, fp_err, fp_measure, plan) == WM_OK);
		FP_CHECK(fp_calls == 0 && plan.dj[0].q_base == 85 && plan.dj[0].t_base == 0 && plan.dj[1].q_base == 0 && plan.dj[1].t_base == 87);
	}
	{   // one step past each edge: job 1 of three is refused with WM_EINVAL and named, job 0 is planned, job 2 is not
		const FinalView wide = { (size_t)1 << 31, seq_len, seq_off, 2 };
		struct { wm_extra_pos_t bad; const FinalView *v; const char *what; } const cases[] = {
			{ { 100, 50, -17, 0, 0, 0, 3 }, &view, "query bases" },                 // q_pos == -17
			{ { 100, 50, 102, 0, 0, 0, 3 }, &view, "query bases" },                 // q_pos + qlen == 2 * qwin_len + 17
			{ { 100, 50, 0, 1, 288, 0, 3 }, &view, "target bases" },                // t_pos + tlen == seq_len[rid] + 1
			{ { 951, 50, 0, 0, 0, 0, 3 }, &view, "resident reads" },                // qwin_off + qwin_len == reads_bytes + 1
			{ { 100, 50, 0, 2, 0, 0, 3 }, &view, "target bases" },                  // rid == n_seq
			{ { 100, 50, 0, -1, 0, 0, 3 }, &view, "target bases" },                 // rid < 0
			{ { 100, 50, 0, 0, -1, 0, 3 }, &view, "target bases" },                 // t_pos < 0
			{ { 0, 1 << 30, 0, 0, 0, 0, 3 }, &wide, "resident reads" },             // qwin_len == 2^30, inside the reads
			{ { 100, 50, 0, 0, 0, 0, -1 }, &view, "CIGAR ops" },                    // nc < 0
			{ { 100, 50, 0, 0, 0, 1, 3 }, &view, "CIGAR ops" } };                   // cig_off + nc == n_ops + 1
		for (const auto &cs : cases) {
			const wm_extra_pos_t pos[3] = { good, cs.bad, good };
			fp_calls = 0; fp_code = 0;
			FP_CHECK(final_plan(*cs.v, 3, 0, 0, pos, cig, 3, 1, LMIN, TILE, fp_err, fp_measure, plan) == WM_EINVAL);
			FP_CHECK(fp_calls == 1 && fp_code == WM_EINVAL && strncmp(fp_msg, "job 1:", 6) == 0 && strstr(fp_msg, cs.what));
			FP_CHECK(plan.order == (std::vector<int>{ 0 }) && plan.tmap.empty() && plan.lmap.empty() && plan.dj.size() == 3 && fp_zero(plan.dj[2]));
			FP_CHECK(plan.dj[0].q_base == 100 && plan.dj[0].n_cigar == 3);
		}
		{   // (the wide view accepts what only its qwin_len rule refused: one less)
			const wm_extra_pos_t pos[1] = { { 0, (1 << 30) - 1, 0, 0, 0, 0, 3 } };
			fp_calls = 0;
			FP_CHECK(final_plan(wide, 1, 0, 0, pos, cig, 3, 1, LMIN, TILE, fp_err, fp_measure, plan) == WM_OK && fp_calls == 0);
		}
		static const wm_extra_job_t bad_bytes[2] = { { 86, 0, 0, 3 }, { 0, 88, 0, 3 } };          // q_off + qlen, t_off + tlen == seqs_bytes + 1
		for (const wm_extra_job_t &bad : bad_bytes) {
			const wm_extra_job_t jobs[3] = { { 0, 0, 0, 3 }, bad, { 0, 0, 0, 3 } };
			fp_calls = 0; fp_code = 0;
			FP_CHECK(final_plan(view, 3, jobs, 100, 0, cig, 3, 1, LMIN, TILE, fp_err, fp_measure, plan) == WM_EINVAL);
			FP_CHECK(fp_calls == 1 && fp_code == WM_EINVAL && strncmp(fp_msg, "job 1:", 6) == 0 && strstr(fp_msg, "more than seqs holds"));
			FP_CHECK(plan.order == (std::vector<int>{ 0 }) && plan.tmap.empty() && plan.lmap.empty() && fp_zero(plan.dj[2]));
		}
	}
	{   // a measure that refuses job 1 wins over job 1's bad operand and loses to its bad CIGAR range
		int measured = 0;
		auto refuses = [&](int i, const uint32_t *cg, int nc, int64_t *qlen, int64_t *tlen, int64_t *cols) {
			++measured;
			if (i == 1) return fp_err(WM_EINVAL, "job %d: the measure refuses", i);
			return fp_measure(i, cg, nc, qlen, tlen, cols);
		};
		const wm_extra_pos_t bad_operand[3] = { good, { 100, 50, -17, 0, 0, 0, 3 }, good }, bad_range[3] = { good, { 100, 50, 0, 0, 0, 1, 3 }, good };
		fp_calls = 0;
		FP_CHECK(final_plan(view, 3, 0, 0, bad_operand, cig, 3, 1, LMIN, TILE, fp_err, refuses, plan) == WM_EINVAL);
		FP_CHECK(fp_calls == 1 && measured == 2 && strcmp(fp_msg, "job 1: the measure refuses") == 0);
		FP_CHECK(plan.order == (std::vector<int>{ 0 }) && fp_zero(plan.dj[1]) && fp_zero(plan.dj[2]) && plan.n_pre == 4);
		fp_calls = 0; measured = 0;
		FP_CHECK(final_plan(view, 3, 0, 0, bad_range, cig, 3, 1, LMIN, TILE, fp_err, refuses, plan) == WM_EINVAL);
		FP_CHECK(fp_calls == 1 && measured == 1 && strncmp(fp_msg, "job 1: CIGAR ops", 16) == 0);
	}
	{   // the tile cap: refused before the job's tiles go in (the columns are claimed by the measure; no CIGAR is that long)
		static const int64_t claimed[2] = { 128, 64 * (((int64_t)1 << 28) - 2) };
		auto claims = [&](int i, const uint32_t*, int, int64_t*, int64_t*, int64_t *cols) { *cols = claimed[i]; return 0; };
		const wm_extra_job_t jobs[2] = { { 0, 0, 0, 1 }, { 0, 0, 0, 1 } };
		fp_calls = 0; fp_code = 0;
		FP_CHECK(final_plan(view, 2, jobs, 1000, 0, cig, 3, 1, LMIN, TILE, fp_err, claims, plan) == WM_ENOMEM);
		FP_CHECK(fp_calls == 1 && fp_code == WM_ENOMEM && strstr(fp_msg, "2^28 tiles"));
		FP_CHECK(fp_pairs(plan.tmap, { { 0, 0 }, { 0, 1 } }) && fp_pairs(plan.lmap, { { 0, 2 } }) && plan.tmap.capacity() < 1024 && plan.order.empty());
		auto claims_all = [&](int, const uint32_t*, int, int64_t*, int64_t*, int64_t *cols) { *cols = 64 * ((int64_t)1 << 28); return 0; };
		fp_calls = 0;
		FP_CHECK(final_plan(view, 1, jobs, 1000, 0, cig, 3, 1, LMIN, TILE, fp_err, claims_all, plan) == WM_ENOMEM);
		FP_CHECK(fp_calls == 1 && plan.tmap.empty() && plan.lmap.empty() && plan.tmap.capacity() < 1024);
	}
	return 0;
}

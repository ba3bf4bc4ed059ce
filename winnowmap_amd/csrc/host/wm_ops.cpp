// wm_ops.cpp — DeviceOps::window_batch composed from the per-operation batches, the host forms of DeviceOps::extra_batch / fix_extra_batch and the switches + accounts of
// the deferred final scans (see wm_ops.h).
#include "wm_ops.h"
#include "wm_sdust.h"
#include "../cigar_fix.h"
#include "../cigar_eqx.h"
#include "../cigar_cs.h"
#include "wm_index.h"
#include "wm_align.h"

namespace wm {

void DeviceOps::window_batch(int w, int k, std::vector<WindowReq*> &reqs)
{
	const size_t n = reqs.size();
	std::vector<SketchReq> sk(n);
	std::vector<SketchReq*> skp;
	for (size_t i = 0; i < n; ++i)
		if (reqs[i]->len > 0) { sk[i].seq = reqs[i]->seq; sk[i].len = reqs[i]->len; sk[i].dev_off = reqs[i]->dev_off; skp.push_back(&sk[i]); }
	if (!skp.empty()) sketch_batch(w, k, skp);
	for (size_t i = 0; i < n; ++i)                   // -T: collect_minimizers' squeeze (src/map.c:80-81), per request
		if (reqs[i]->len > 0 && reqs[i]->sdust_thres > 0) dust_minimizers(sk[i].mini, reqs[i]->seq, reqs[i]->len, reqs[i]->sdust_thres);
	// collect_seed_hits takes one (max_occ, flag) per batch: group the requests (one group in practice)
	std::vector<SeedReq> sd(n);
	std::vector<char> done(n, 0);
	for (size_t i = 0; i < n; ++i) {
		if (done[i] || reqs[i]->len <= 0 || sk[i].mini.empty()) continue;
		std::vector<SeedReq*> grp;
		for (size_t j = i; j < n; ++j)
			if (!done[j] && reqs[j]->len > 0 && !sk[j].mini.empty() && reqs[j]->max_occ == reqs[i]->max_occ && reqs[j]->flag == reqs[i]->flag) {
				sd[j].mini = sk[j].mini.data(); sd[j].n_mini = (int)sk[j].mini.size(); sd[j].qlen = reqs[j]->len; sd[j].max_occ = reqs[j]->max_occ; sd[j].flag = reqs[j]->flag;
				sd[j].has_key = reqs[j]->has_key; sd[j].q_lo = reqs[j]->q_lo; sd[j].q_eq = reqs[j]->q_eq;
				grp.push_back(&sd[j]); done[j] = 1;
			}
		seed_batch(grp);
	}
	std::vector<ChainReq> ch(n);
	std::vector<ChainReq*> chp;
	for (size_t i = 0; i < n; ++i) {
		WindowReq &r = *reqs[i];
		ChainReq &c = ch[i];
		c.a = std::move(r.pre);
		r.rep_len = sd[i].rep_len;
		if (r.len > 0) {
			const bool both = !c.a.empty();
			c.a.insert(c.a.end(), sd[i].a.begin(), sd[i].a.end());
			if (both) radix_sort_128x(c.a.data(), c.a.data() + c.a.size());       // src/map.c:833
		}
		r.n_anchors = (int)c.a.size();
		c.max_dist_x = r.max_dist_x; c.min_dist_x = r.min_dist_x; c.max_dist_y = r.max_dist_y; c.bw = r.bw; c.max_skip = r.max_skip; c.max_iter = r.max_iter;
		c.min_cnt = r.min_cnt; c.min_sc = r.min_sc; c.gap_scale = r.gap_scale; c.is_cdna = r.is_cdna;
		if (!c.a.empty()) chp.push_back(&c);
	}
	if (!chp.empty()) chain_batch(chp);
	for (size_t i = 0; i < n; ++i) {
		WindowReq &r = *reqs[i];
		if (r.n_anchors > 0) { r.a = std::move(ch[i].a); r.u = std::move(ch[i].u); } else { r.a.clear(); r.u.clear(); }
	}
}

// ---- the scan of mm_update_extra as a deferred, batched operation ----------------------------------------------------------------------------
static DevSwitch g_extra_dev{"WM_EXTRA_DEV"};
bool extra_device_on() { return g_extra_dev.on(); }
ExtraStats &extra_stats() { static ExtraStats s; return s; }

void DeviceOps::extra_batch(const wm_extra_score_t &sc, std::vector<ExtraReq*> &reqs)
{
	WM_SITE("extra.host_walk");
	parallel_for(1, reqs.size(), [&](size_t i) {
		ExtraReq &r = *reqs[i];
		extra_walk_host(r.qp, r.tp, r.cigar, r.n_cigar, sc.match, sc.mismatch, sc.ambi, sc.q, sc.e, &r.out);
		if (r.eqx) eqx_host(*r.eqx, r.qp, r.tp);                                 // src/align.c:285
	});
	extra_stats().on_host += reqs.size();
}

// ---- mm_fix_cigar + the scan as one deferred, batched operation -------------------------------------------------------------------------------
static DevSwitch g_fix_dev{"WM_FIX_DEV"};
bool fix_device_on() { return g_fix_dev.on(); }
FixStats &fix_stats() { static FixStats s; return s; }

void DeviceOps::fix_extra_batch(const wm_extra_score_t &sc, std::vector<FixReq*> &reqs)
{
	WM_SITE("fix.host");
	parallel_for(1, reqs.size(), [&](size_t i) {
		FixReq &r = *reqs[i];
		int n = (int)r.cigar->size(), qs = 0, ts = 0;
		if (n > 1) { wm_fix_cigar(r.cigar->data(), &n, r.qp, r.tp, &qs, &ts, 0, 0); r.cigar->resize((size_t)n); }
		r.qshift = qs; r.tshift = ts;
		extra_walk_host(r.qp + qs, r.tp + ts, r.cigar->data(), n, sc.match, sc.mismatch, sc.ambi, sc.q, sc.e, &r.out);
		if (r.eqx) eqx_host(*r.cigar, r.qp + qs, r.tp + ts);                     // src/align.c:285
	});
	fix_stats().on_host += reqs.size();
}

// ---- mm_update_cigar_eqx: the host form, and the deferred, batched operation ----------------------------------------------------------------------
int eqx_host(std::vector<uint32_t> &cigar, const uint8_t *qseq, const uint8_t *tseq)
{
	const int n = (int)cigar.size();
	uint32_t n_M;
	const uint32_t n_EQX = wm_cigar_eqx_count(cigar.data(), n, qseq, tseq, &n_M);
	if (n_EQX == n_M) { wm_cigar_eqx_relabel(cigar.data(), n, cigar.data()); return 1; }
	std::vector<uint32_t> out((size_t)n - n_M + n_EQX);
	const int m = wm_cigar_eqx_rewrite(cigar.data(), n, qseq, tseq, out.data());
	WM_INVARIANT((size_t)m == out.size());
	cigar.swap(out);
	return 0;
}
static DevSwitch g_eqx_dev{"WM_EQX_DEV"};
bool eqx_device_on() { return g_eqx_dev.on(); }
EqxStats &eqx_stats() { static EqxStats s; return s; }

void DeviceOps::eqx_batch(std::vector<EqxReq*> &reqs)
{
	WM_SITE("eqx.host");
	parallel_for(1, reqs.size(), [&](size_t i) {
		EqxReq &r = *reqs[i];
		r.in_place = eqx_host(*r.cigar, r.qp, r.tp) != 0;
	});
	eqx_stats().on_host += reqs.size();
}

// ---- the cs:Z / MD:Z bodies: the host form, and the deferred, batched operation ---------------------------------------------------------------------
void cs_body_host(const Index &idx, const char *seq, int32_t rid, int32_t rs, int32_t re, int32_t qs, int32_t qe, bool rev, const std::vector<uint32_t> &cigar, int mode, std::string &out)
{   // write_cs_or_MD, src/format.c:220-243
	const int ql = qe - qs, tl = re - rs;
	std::vector<uint8_t> tseq(tl > 0 ? tl : 1), qseq(ql > 0 ? ql : 1);
	if (tl > 0) idx.getseq(rid, rs, re, tseq.data());
	for (int i = qs; i < qe; ++i) {
		const uint8_t c = nt4_table[(uint8_t)seq[i]];
		if (!rev) qseq[i - qs] = c;
		else qseq[qe - i - 1] = c >= 4 ? 4 : 3 - c;
	}
	const size_t at = out.size();
	out.resize(at + (size_t)wm_cigar_cs_bound(cigar.data(), (int)cigar.size()));
	const int64_t n = wm_cigar_cs(mode, cigar.data(), (int)cigar.size(), qseq.data(), tseq.data(), &out[at]);
	WM_INVARIANT(n >= 0);                       // (the asserts of src/format.c:147, :180, :195)
	out.resize(at + (size_t)(n > 0 ? n : 0));
}
static DevSwitch g_cs_dev{"WM_CS_DEV"};
bool cs_device_on() { return g_cs_dev.on(); }
CsStats &cs_stats() { static CsStats s; return s; }

void DeviceOps::cs_batch(std::vector<CsReq*> &reqs)
{
	WM_SITE("cs.host");
	parallel_for(1, reqs.size(), [&](size_t i) {
		CsReq &r = *reqs[i];
		r.body->clear();
		cs_body_host(*r.idx, r.seq, r.rid, r.rs, r.re, r.qs, r.qe, r.rev, *r.cigar, r.mode, *r.body);
	});
	cs_stats().on_host += reqs.size();
}

// ---- ksw_ll_i16 as a batched operation: requests that travel through the alignment queue (KswReq::local) -------------------------------------------------
static DevSwitch g_ll_dev{"WM_LL_DEV"};
bool ll_device_on() { return g_ll_dev.on(); }
LlStats &ll_stats() { static LlStats s; return s; }

void DeviceOps::ll_batch(const int8_t *mat5x5, int gapo, int gape, std::vector<KswReq*> &reqs)
{
	WM_SITE("ll.host");
	parallel_for(1, reqs.size(), [&](size_t i) {
		KswReq &r = *reqs[i];
		int qe = -1, te = -1;
		if (r.step == 1) r.ez.max = ll_i16(r.ql, r.qp, r.tl, r.tp, mat5x5, gapo, gape, &qe, &te);
		else {
			std::vector<uint8_t> q(r.ql > 0 ? r.ql : 1), t(r.tl > 0 ? r.tl : 1);
			r.copy_query(q.data()); r.copy_target(t.data());
			r.ez.max = ll_i16(r.ql, q.data(), r.tl, t.data(), mat5x5, gapo, gape, &qe, &te);
		}
		r.ez.max_q = qe; r.ez.max_t = te;
	});
	ll_stats().on_host += reqs.size();
}

// ---- the accounts of the five switches: the C entry points' copy-out, and the lines at unload --------------------------------------------------------
typedef std::initializer_list<std::atomic<uint64_t>*> StatFields;      // an account's counters in the order its entry point documents (include/wm_gpu.h)
static void take_stats(StatFields f, uint64_t *out, int reset)
{
	size_t i = 0;
	for (std::atomic<uint64_t> *a : f) { if (out) out[i] = a->load(); if (reset) a->store(0); ++i; }
}
// WM_EXTRA_REPORT=1: the accounts on stderr when the library is unloaded (a front end that is not ours — the benchmark — has no other way to ask); an account
// with nothing deferred prints nothing. Every '#' of `text` is the next counter.
static void report_line(const char *text, StatFields f)
{
	if (!(*f.begin())->load()) return;
	std::string line;
	const std::atomic<uint64_t> *const *next = f.begin();
	for (const char *p = text; *p; ++p) { if (*p == '#') line += std::to_string((*next++)->load()); else line += *p; }
	fputs(line.c_str(), stderr);
}
static struct AccountReport {
	~AccountReport()
	{
		if (!getenv("WM_EXTRA_REPORT")) return;
		CsStats &c = cs_stats(); FixStats &f = fix_stats(); EqxStats &q = eqx_stats(); ExtraStats &x = extra_stats(); LlStats &l = ll_stats();
		report_line("[wm] ll: # jobs deferred, # served on the device, # on the host, # batched calls, # cells, # us inside the calls\n",
		            { &l.deferred, &l.on_device, &l.on_host, &l.calls, &l.cells, &l.us });
		report_line("[wm] cs: # regions deferred, # served on the device, # on the host, # batched calls, # bytes, # us inside the calls\n",
		            { &c.deferred, &c.on_device, &c.on_host, &c.calls, &c.bytes, &c.us });
		report_line("[wm] fix: # regions deferred, # fixed on the device, # on the host, # early on the host (inversion test), # batched calls, # us inside the calls, # columns\n",
		            { &f.deferred, &f.on_device, &f.on_host, &f.early, &f.calls, &f.us, &f.cols });
		report_line("[wm] eqx: # regions deferred, # rewritten on the device, # on the host, # batched calls, # M columns, # us inside the calls\n",
		            { &q.deferred, &q.on_device, &q.on_host, &q.calls, &q.cols, &q.us });
		report_line("[wm] extra: # regions deferred, # walked on the device, # on the host, # batched calls, # columns, # us inside the calls\n",
		            { &x.deferred, &x.on_device, &x.on_host, &x.calls, &x.cols, &x.us });
	}
} g_account_report;

} // namespace wm

extern "C" {
void wm_set_fix_device(int on) { wm::g_fix_dev.set(on); }
int wm_fix_device_enabled(void) { return wm::fix_device_on() ? 1 : 0; }
void wm_fix_stats(uint64_t *out7, int reset) { wm::FixStats &s = wm::fix_stats(); wm::take_stats({ &s.deferred, &s.on_device, &s.on_host, &s.early, &s.calls, &s.us, &s.cols }, out7, reset); }
void wm_set_cs_device(int on) { wm::g_cs_dev.set(on); }
int wm_cs_device_enabled(void) { return wm::cs_device_on() ? 1 : 0; }
void wm_cs_stats(uint64_t *out6, int reset) { wm::CsStats &s = wm::cs_stats(); wm::take_stats({ &s.deferred, &s.on_device, &s.on_host, &s.calls, &s.bytes, &s.us }, out6, reset); }
void wm_set_eqx_device(int on) { wm::g_eqx_dev.set(on); }
int wm_eqx_device_enabled(void) { return wm::eqx_device_on() ? 1 : 0; }
void wm_eqx_stats(uint64_t *out6, int reset) { wm::EqxStats &s = wm::eqx_stats(); wm::take_stats({ &s.deferred, &s.on_device, &s.on_host, &s.calls, &s.cols, &s.us }, out6, reset); }
void wm_set_ll_device(int on) { wm::g_ll_dev.set(on); }
int wm_ll_device_enabled(void) { return wm::ll_device_on() ? 1 : 0; }
void wm_ll_stats(uint64_t *out6, int reset) { wm::LlStats &s = wm::ll_stats(); wm::take_stats({ &s.deferred, &s.on_device, &s.on_host, &s.calls, &s.cells, &s.us }, out6, reset); }
void wm_set_extra_device(int on) { wm::g_extra_dev.set(on); }
int wm_extra_device_enabled(void) { return wm::extra_device_on() ? 1 : 0; }
void wm_extra_stats(uint64_t *out6, int reset) { wm::ExtraStats &s = wm::extra_stats(); wm::take_stats({ &s.deferred, &s.on_device, &s.on_host, &s.calls, &s.cols, &s.us }, out6, reset); }
}

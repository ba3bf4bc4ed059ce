// wm_ops.h — the batched device operations the host mapper is written against. The product wires the HIP
// implementation (GpuOps in wm_gpu.hip → libwmgpu kernels). The interface exists so that the host glue can be
// exercised by the test-suite with a checker-backed implementation (tests/host_harness) on a machine with no GPU;
// nothing in the product constructs anything but GpuOps.
#pragma once
#include "wm_core.h"
#include "../cigar_walk.h"
#include <atomic>
#include <stdlib.h>
#include <string>
#include <vector>

namespace wm {

// Sequences the mapper hands to the device exist twice: as host views (plain pointers to 0..4 codes, used by the host-side judge /
// finish code and by checker-backed implementations) and as POSITIONS in data the device already holds — the codes of the whole
// mini-batch, uploaded once by DeviceOps::load_reads, and the packed reference uploaded with the index — so that a device
// implementation never has to copy, pack or ship a sequence per request. dev_off < 0: the sequence is not resident (use the view).
struct SketchReq {                 // mm_sketch of one (sub)sequence of 0..4 codes, rid = 0
	const uint8_t *seq = 0; int len = 0;
	int64_t dev_off = -1;          // offset of seq[0] in the resident read codes
	std::vector<m128> mini;        // out
};

struct SeedReq {                   // collect_seed_hits (src/map.c:222-254): lookup, occ filter, expand, sort by x
	const m128 *mini = 0; int n_mini = 0; int qlen = 0; int max_occ = 0; int64_t flag = 0;
	std::vector<m128> a;           // out: anchors sorted with radix_sort_128x
	int rep_len = 0;               // out (src/map.c:111-116,126)
	// name key of the query for this index (Index::name_key): with it F_NO_DIAG / F_NO_DUAL in `flag` are served (skip_seed, src/map.c:132-154);
	// without it they are ignored, as the reference ignores them for qname == NULL
	bool has_key = false; uint32_t q_lo = 0, q_eq = 0;
};

struct ChainReq {                  // mm_chain_dp (src/chain.c:22); consumes `a`
	int max_dist_x = 0, min_dist_x = 0, max_dist_y = 0, bw = 0, max_skip = 0, max_iter = 0, min_cnt = 0, min_sc = 0;
	float gap_scale = 1.0f;
	bool is_cdna = false;          // splice mode: an intron-sized reference gap costs min(linear, log) (src/chain.c:69-74)
	std::vector<m128> a;           // in: sorted anchors; out: anchors grouped by chain
	std::vector<uint64_t> u;       // out: score<<32 | count per chain
};

// One MCAS window or stage-2 pass from the sequence to the chains (src/map.c:69-84, 222-254, 375-430; src/chain.c:22-167): mm_sketch of
// `seq` (if any), collect_seed_hits, the handed-in anchors `pre` (stage 2: what stage 1 collected, already sorted) in front of the seeded
// ones and the union sorted again when both are present (src/map.c:818-833), then mm_chain_dp. A device implementation keeps everything
// between the codes and the chains in HBM (wm_window_batch).
struct WindowReq {
	const uint8_t *seq = 0; int len = 0;   // 0..4 codes (host view); len == 0: no sequence, only `pre` is chained
	int64_t dev_off = -1;                  // offset of seq[0] in the resident read codes, -1 = not resident (the view is staged)
	std::vector<m128> pre;                 // in
	int max_occ = 0; int64_t flag = 0;     // collect_seed_hits
	int sdust_thres = 0;                   // > 0: mm_dust_minier squeezes the minimizers before the seeding (src/map.c:43-67, 80-81)
	int max_dist_x = 0, min_dist_x = 0, max_dist_y = 0, bw = 0, max_skip = 0, max_iter = 0, min_cnt = 0, min_sc = 0;   // mm_chain_dp
	float gap_scale = 1.0f;
	bool is_cdna = false;
	std::vector<m128> a;                   // out: anchors grouped by chain
	std::vector<uint64_t> u;               // out: score<<32 | count per chain
	int rep_len = 0, n_anchors = 0;        // out: src/map.c:126; anchors before chaining
	bool has_key = false; uint32_t q_lo = 0, q_eq = 0;   // name key of the read, as SeedReq; the length skip_seed compares is `len` (a window's inside stage 1)
};

struct KswReq {                    // ksw_extd2_sse (src/ksw2.h:60)
	// host views: element i of the query is qp[i * step], of the target tp[i * step]; step = -1 for the left extension, which aligns
	// both sequences reversed (src/align.c:690-705). Valid while the request is pending.
	const uint8_t *qp = 0, *tp = 0;
	int32_t ql = 0, tl = 0, step = 1;
	// the same operands as positions in resident data. Query: index q_pos of the TWO-STRAND SPACE of the (sub)read that starts at
	// qwin_off and is qwin_len long — [0, L) forward strand, [L, 2L) reverse complement, negative = N padding; this is the layout of the
	// reference's qseq0 buffer (src/align.c:871-877), including the few bases in front of a strand that mm_align1_inv may touch.
	// Target: base t_pos of contig rid. has_n: an operand may contain an ambiguous base (conservative).
	int64_t qwin_off = -1; int32_t qwin_len = 0, q_pos = 0, rid = -1, t_pos = 0;
	bool has_n = true;
	int w = 0, zdrop = 0, end_bonus = 0, flag = 0;
	// splice mode with a junction annotation (--junc-bed): the bits of mm_idx_bed_junc (src/index.c:768-803) for the target range, in the
	// order the target is presented (reversed for the left extension, src/align.c:693-696); empty = no annotation
	std::vector<uint8_t> junc;
	// want_zd: the mapper will judge this alignment's z-drop (mm_test_zdrop, src/align.c:32-89) — a device implementation may return the scan with the
	// alignment (has_zd + zd, see cigar_walk.h); without it the host walks the CIGAR itself
	bool want_zd = false, has_zd = false;
	wm_zd_t zd = { 0, -1, -1, -1, -1 };
	// local: not an extension but ksw_ll_qinit + ksw_ll_i16 (src/ksw2.h:82-83) on the same operands — the inversion test, mm_align1_inv's placement, the splice end
	// filter, filed while the switch of wm_set_ll_device is on. w, zdrop, end_bonus and flag are ignored; ez.max = the score, ez.max_q = qe, ez.max_t = te (the
	// striped machine's, csrc/ksw_ll.h); there is no CIGAR. The hub hands such requests to DeviceOps::ll_batch: ksw_batch / exts2_batch never see one.
	bool local = false;
	wm_ksw_result_t ez = {};       // out
	std::vector<uint32_t> cigar;   // out
	int qlen() const { return ql; }
	int tlen() const { return tl; }
	bool resident() const { return qwin_off >= 0 && rid >= 0; }
	void copy_query(uint8_t *dst) const { for (int i = 0; i < ql; ++i) dst[i] = qp[(ptrdiff_t)i * step]; }
	void copy_target(uint8_t *dst) const { for (int i = 0; i < tl; ++i) dst[i] = tp[(ptrdiff_t)i * step]; }
};

struct ExtraReq {                  // the scan of mm_update_extra (src/align.c:240-286) over a region's FINAL CIGAR (after mm_fix_cigar, forward order)
	// host views of both operands from the alignment's first base on, readable 16 bytes beyond the aligned stretch; valid while the request is pending
	const uint8_t *qp = 0, *tp = 0;
	// the same operands as positions in resident data, the rule of KswReq without a step: two-strand index q_pos of the (sub)read at qwin_off / qwin_len
	// (mm_align1_inv's region may start a few bases in front of its strand: the tail of the other strand, or N padding), base t_pos of contig rid
	int64_t qwin_off = -1; int32_t qwin_len = 0, q_pos = 0, rid = -1, t_pos = 0;
	const uint32_t *cigar = 0; int n_cigar = 0;            // the region's CIGAR (stays where it is until the request is served)
	wm_extra_score_t sc = { 0, 0, 0, 0, 0 };               // mat[0], mat[1], mat[24], opt->q, opt->e: one value per mapping call
	wm_extra_t out = { 0, 0, 0, 0, 0, 0 };                 // out
	// MM_F_EQX with the rewriting not deferred (EqxReq below): the region's own vector (the same ops `cigar` points at), rewritten by mm_update_cigar_eqx
	// (src/align.c:169-238, csrc/cigar_eqx.h) right after the scan, as the reference does (:285); 0 = no rewriting
	std::vector<uint32_t> *eqx = 0;
	bool resident() const { return qwin_off >= 0 && rid >= 0; }
};
struct FixReq {                    // mm_update_extra as a whole (src/align.c:240-286): mm_fix_cigar (:91-167) on a region's STITCHED CIGAR, then the scan of what it leaves
	// host views and positions of both operands from the first base of the STITCHED alignment on, the rules of ExtraReq
	const uint8_t *qp = 0, *tp = 0;
	int64_t qwin_off = -1; int32_t qwin_len = 0, q_pos = 0, rid = -1, t_pos = 0;
	std::vector<uint32_t> *cigar = 0;                      // in: the stitched CIGAR; out: the fixed one (the region's own vector)
	wm_extra_score_t sc = { 0, 0, 0, 0, 0 };
	int32_t qshift = 0, tshift = 0;                        // out: the leading I / D that went (the mapper moves qs / qe / rs)
	wm_extra_t out = { 0, 0, 0, 0, 0, 0 };                 // out: the scan of the fixed CIGAR, operands advanced by both shifts
	bool eqx = false;                                      // MM_F_EQX, not deferred: mm_update_cigar_eqx on the fixed CIGAR after the scan (src/align.c:285), operands advanced by both shifts
	bool resident() const { return qwin_off >= 0 && rid >= 0; }
};
struct EqxReq {                    // mm_update_cigar_eqx (src/align.c:169-238) over a region's FINAL CIGAR, deferred (the switch of wm_set_eqx_device): M -> runs of = / X
	// host views and positions of both operands from the alignment's first base on, advanced by both shifts of mm_fix_cigar: the rules of ExtraReq
	const uint8_t *qp = 0, *tp = 0;
	int64_t qwin_off = -1; int32_t qwin_len = 0, q_pos = 0, rid = -1, t_pos = 0;
	std::vector<uint32_t> *cigar = 0;                      // in: the final CIGAR; out: the rewritten one (the region's own vector)
	int32_t cap_hint = 0;                                  // ops the result can have at most: n_ops + 2 x (blen - mlen + n_ambi) of the finished scan, every unequal column a run of its own plus the split it causes
	bool in_place = false;                                 // out: the branch of src/align.c:195-201 ran
	bool resident() const { return qwin_off >= 0 && rid >= 0; }
};
struct Index;
struct CsReq {                     // the body of a region's cs:Z / MD:Z tag (write_cs_core / write_MD_core, src/format.c:141-218), produced when the read's regions are final (the switch of wm_set_cs_device)
	// the host form prepares its operands as write_cs_or_MD does (:220-243): the region's target through mm_idx_getseq, its query strand from the read's characters
	const Index *idx = 0; const char *seq = 0;            // the index; the read as it came in
	int32_t rid = -1, rs = 0, re = 0, qs = 0, qe = 0; bool rev = false;
	// the device form reads the resident read (two-strand space: q_pos = qs, or 2 * qwin_len - qe on the reverse strand) and the uploaded reference from rs on
	int64_t qwin_off = -1; int32_t qwin_len = 0, q_pos = 0;
	const std::vector<uint32_t> *cigar = 0;                // the region's final CIGAR
	int mode = 0;                                          // WM_CS_SHORT / WM_CS_LONG / WM_CS_MD (csrc/cigar_cs.h)
	std::string *body = 0;                                 // out: the tag's body, without its "\tcs:Z:" / "\tMD:Z:"
	bool resident() const { return qwin_off >= 0 && rid >= 0; }
};
// the body of one region's tag on the host: the operand preparation of write_cs_or_MD (src/format.c:220-243), then wm_cigar_cs (csrc/cigar_cs.h); appended to `out`
void cs_body_host(const Index &idx, const char *seq, int32_t rid, int32_t rs, int32_t re, int32_t qs, int32_t qe, bool rev, const std::vector<uint32_t> &cigar, int mode, std::string &out);
// mm_update_cigar_eqx on a vector (csrc/cigar_eqx.h); returns 1 if the in-place branch ran
int eqx_host(std::vector<uint32_t> &cigar, const uint8_t *qseq, const uint8_t *tseq);
// wm_extra_walk (csrc/cigar_walk.h), 16 bases per step where the build has SSE2 and match > 0 (host/wm_align.cpp)
void extra_walk_host(const uint8_t *qseq, const uint8_t *tseq, const uint32_t *cigar, int n_cigar, int match, int mismatch, int ambi, int q, int e, wm_extra_t *out);

// An opt-in switch of the mapper: what wm_set_X_device last said, or, while that is -1, what the variable `env` says whenever a mapping call starts.
struct DevSwitch {
	const char *env;
	std::atomic<int> v{-1};
	bool on() const
	{
		const int x = v.load(std::memory_order_relaxed);
		if (x >= 0) return x != 0;
		const char *e = getenv(env);
		return e && atoi(e) != 0;
	}
	void set(int on_) { v = on_ < 0 ? -1 : on_ ? 1 : 0; }
};

// The mapper's switch for that scan (wm_set_extra_device / WM_EXTRA_DEV, include/wm_gpu.h; off by default) and its process-wide account (wm_extra_stats). They live
// with the host mapper, so the test harness has them too.
bool extra_device_on();
struct ExtraStats { std::atomic<uint64_t> deferred{0}, on_device{0}, on_host{0}, calls{0}, cols{0}, us{0}; };
ExtraStats &extra_stats();

// The switch for BOTH halves (wm_set_fix_device / WM_FIX_DEV; off by default) and its account (wm_fix_stats): regions whose fix was deferred, fixed on the device, fixed
// on the host by the batched request, fixed on the host early because an inversion test was about to read them, batched device calls, microseconds inside them, alignment columns the fused calls walked.
bool fix_device_on();
struct FixStats { std::atomic<uint64_t> deferred{0}, on_device{0}, on_host{0}, early{0}, calls{0}, us{0}, cols{0}; };
FixStats &fix_stats();

// The switch for the = / X rewriting under MM_F_EQX (wm_set_eqx_device / WM_EQX_DEV; off by default) and its account (wm_eqx_stats): regions deferred, rewritten on the
// device, rewritten on the host by the batched request, batched device calls, M columns those calls walked, microseconds inside them.
bool eqx_device_on();
struct EqxStats { std::atomic<uint64_t> deferred{0}, on_device{0}, on_host{0}, calls{0}, cols{0}, us{0}; };
EqxStats &eqx_stats();

// The switch for the cs:Z / MD:Z bodies under MM_F_OUT_CS / MM_F_OUT_MD (wm_set_cs_device / WM_CS_DEV; off by default) and its account (wm_cs_stats): regions deferred,
// served on the device, served on the host by the batched request, batched device calls, bytes they produced, microseconds inside them.
bool cs_device_on();
struct CsStats { std::atomic<uint64_t> deferred{0}, on_device{0}, on_host{0}, calls{0}, bytes{0}, us{0}; };
CsStats &cs_stats();

// The switch for ksw_ll_i16 (wm_set_ll_device / WM_LL_DEV; off by default) and its account (wm_ll_stats): jobs deferred, served on the device, served on the host by the
// batched request, batched device calls, DP cells of those calls, microseconds inside them.
bool ll_device_on();
struct LlStats { std::atomic<uint64_t> deferred{0}, on_device{0}, on_host{0}, calls{0}, cells{0}, us{0}; };
LlStats &ll_stats();

// The batch calls are synchronous (they return when the results are in the requests) and must be callable from several threads at
// once: the hub (wm_fiber.h) keeps up to max_inflight() of them running concurrently.
struct DeviceOps {
	virtual ~DeviceOps() {}
	virtual int max_inflight() const { return 1; }
	// true if a thread inside a batched call mostly sleeps (waiting for the device): the mapper then runs that many workers more than cores
	virtual bool waits_asleep() const { return false; }
	// the 0..4 codes of every read of the mini-batch, back to back (SketchReq::dev_off / KswReq::qwin_off index this buffer). Returns
	// true if the implementation keeps them resident; false = requests must be served from their host views.
	// `slot` (0 or 1): two mini-batches may be mapped concurrently by two calls that share one DeviceOps (the start-up and drain phases of one
	// hide behind the other); each keeps its codes in its own slab and adds *base to its offsets. release_reads: the call is over.
	virtual bool load_reads(const uint8_t *codes, size_t n, int slot, int64_t *base) { (void)codes; (void)n; (void)slot; *base = 0; return false; }
	virtual void release_reads(int slot) { (void)slot; }
	virtual void sketch_batch(int w, int k, std::vector<SketchReq*> &reqs) = 0;
	virtual void seed_batch(std::vector<SeedReq*> &reqs) = 0;
	virtual void chain_batch(std::vector<ChainReq*> &reqs) = 0;
	virtual void ksw_batch(const wm_ksw_score_t &sc, std::vector<KswReq*> &reqs) = 0;
	// splice mode: the same requests through ksw_exts2_sse (src/align.c:326-327) — no band, no end bonus, sc.q2 = the price of an intron;
	// KswReq::flag carries the KSW_EZ_SPLICE_* bits. No junction annotation (mm_idx_bed_junc: the BED reader is outside the path).
	virtual void exts2_batch(const wm_ksw_score_t &sc, int noncan, int junc_bonus, std::vector<KswReq*> &reqs) = 0;
	// the local-score requests (KswReq::local, the switch above) that the hub split off the alignment queue. The default runs the specification's host form
	// (wm::ll_i16) on the host views — checker-backed implementations need nothing; the product's GpuOps overrides it with wm_ksw_ll_batch_pos when every request is
	// resident and within WM_LL_MAX_LEN.
	virtual void ll_batch(const int8_t *mat5x5, int gapo, int gape, std::vector<KswReq*> &reqs);
	// the deferred final scans of a mapping call's regions (the switch above). The default walks them on the host (wm_extra_walk / its SSE form) — checker-backed
	// implementations need nothing; the product's GpuOps overrides it with wm_extra_batch_pos when every request is resident.
	virtual void extra_batch(const wm_extra_score_t &sc, std::vector<ExtraReq*> &reqs);
	// ... and both halves of mm_update_extra for regions that kept their stitched CIGAR (the switch above). The default runs the specification (csrc/cigar_fix.h) and the
	// host walk; the product's GpuOps overrides it with wm_fix_extra_batch_pos when every request is resident and the call would not be refused.
	virtual void fix_extra_batch(const wm_extra_score_t &sc, std::vector<FixReq*> &reqs);
	// the deferred = / X rewriting of final CIGARs (MM_F_EQX with the switch above). The default runs the specification (csrc/cigar_eqx.h); the product's GpuOps
	// overrides it with wm_eqx_batch_pos when every request is resident.
	virtual void eqx_batch(std::vector<EqxReq*> &reqs);
	// the bodies of the cs:Z / MD:Z tags of finished reads (MM_F_OUT_CS / MM_F_OUT_MD with the switch above). The default runs the specification (csrc/cigar_cs.h) on
	// operands prepared as the output step prepares them; the product's GpuOps overrides it with wm_cs_batch_pos when every request is resident and none would be refused.
	virtual void cs_batch(std::vector<CsReq*> &reqs);
	// the whole window in one call. The default composes it from the three operations above (checker-backed implementations in the
	// test-suite); the product's GpuOps overrides it with the HBM-resident wm_window_batch.
	virtual void window_batch(int w, int k, std::vector<WindowReq*> &reqs);
};

} // namespace wm

"""GPU: ksw_ll_i16 on the device (csrc/ll_kernel.h behind wm_ksw_ll_batch / wm_ksw_ll_batch_pos; src/ksw2_ll_sse.c:80-147) — every named case in both read directions
under three settings of the class boundary, 300 random jobs, the sizes at which the launch takes another kernel (the two LDS instantiations) and the position form
over uploaded reads and a small uploaded index, all against wm_ksw_ll_i16, the host form the mapper has run so far (tests/test_abi.py pins it to the reference);
the refusals, each with `out` untouched; and the mapper with its ksw_ll_i16 jobs served on the device (wm_set_ll_device), which must give the very hits, CIGARs and
text it gives with the switch off — and the host mapper over the oracle, and the reference where oracle/_ref is built — also with two mapping calls in flight."""
import ctypes as C
import os
import tempfile
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import wmtest as W
import e2e_common as E
import llcases as Q
from winnowmap_amd import build, gpu, synth

pytestmark = pytest.mark.gpu
BOUNDARIES = (Q.REG_MAX_DEFAULT, 32, 0)


@pytest.fixture(scope="module")
def ctx():
    c = gpu.Context(0, 2 << 30)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def restore_switches_and_routing():
    """all process-global: every test leaves the library's defaults behind"""
    assert gpu.ksw_ll_reg_max() == Q.REG_MAX_DEFAULT and gpu.LL_MAX_LEN >= 16000
    try:
        yield
    finally:
        gpu.set_ksw_ll_routing(Q.REG_MAX_DEFAULT)
        gpu.set_ll_device(-1); gpu.set_cs_device(-1); gpu.set_eqx_device(-1); gpu.set_fix_device(-1); gpu.set_extra_device(-1)


def mat_of(c):
    return Q.simple_mat(c["a"], c["b"], c["ambi"])


def host_form(c, rev=False):
    """wm_ksw_ll_i16: the existing host form, not the code under test"""
    L = gpu.lib()
    L.wm_ksw_ll_i16.restype = C.c_int
    L.wm_ksw_ll_i16.argtypes = [C.c_int, W.u8p, C.c_int, W.u8p, W.i8p, C.c_int, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    q, t = (np.ascontiguousarray(c["q"][::-1]), np.ascontiguousarray(c["t"][::-1])) if rev else (c["q"], c["t"])
    qe, te = C.c_int(), C.c_int()
    s = L.wm_ksw_ll_i16(len(q), q, len(t), t, mat_of(c), c["gapo"], c["gape"], C.byref(qe), C.byref(te))
    return s, qe.value, te.value


def groups(cases):
    g = {}
    for i, c in enumerate(cases):
        g.setdefault((c["a"], c["b"], c["ambi"], c["gapo"], c["gape"]), []).append(i)
    return g


def run_bytes(ctx, cases, step):
    got = [None] * len(cases)
    for idx in groups(cases).values():
        part = [cases[i] for i in idx]
        q_off, t_off, ql, tl, st, seqs = Q.pack(part, step)
        jobs = np.zeros(len(part), gpu.LL_JOB_DTYPE)
        jobs["q_off"], jobs["t_off"], jobs["qlen"], jobs["tlen"], jobs["step"] = q_off, t_off, ql, tl, st
        out = ctx.ksw_ll_batch(mat_of(part[0]), part[0]["gapo"], part[0]["gape"], jobs, seqs)
        for i, o in zip(idx, out):
            got[i] = tuple(int(v) for v in o)
    return got


@pytest.fixture(scope="module")
def EXPECTED():
    """computed once: the named cases and the jobs at the launch's other size thresholds, with what the host form gives"""
    rng = np.random.default_rng(9)
    cases = Q.make_cases()
    for ql, tl in ((200, 8192), (200, 8193), (72, gpu.LL_MAX_LEN), (gpu.LL_MAX_LEN, 70)):      # the 64 KB | 128 KB instantiations of the LDS class; the limit itself
        q = rng.integers(0, 4, ql).astype(np.uint8)
        t = rng.integers(0, 4, tl).astype(np.uint8)
        n = min(ql, tl) - 8
        t[tl - n - 3:tl - 3] = q[:n]                          # the query's copy ends near the target's end: the hand-over rows far down are used
        cases.append(Q.case("lds_q%d_t%d" % (ql, tl), q, t))
    q = rng.integers(0, 4, 5000).astype(np.uint8)
    cases.append(Q.case("big_5000_x_5000", q, Q._related(rng, q, 5000, 0.1, 0.04)))
    return cases, [host_form(c) for c in cases]


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("reg_max", BOUNDARIES)
@pytest.mark.parametrize("step", [1, -1])
def test_every_named_case_equals_the_host_form(ctx, EXPECTED, step, reg_max):
    gpu.set_ksw_ll_routing(reg_max)
    assert gpu.ksw_ll_reg_max() == reg_max
    cases, want = EXPECTED
    got = run_bytes(ctx, cases, step)
    for c, w, g in zip(cases, want, got):
        assert g == w, (c["name"], step, reg_max, g, w)
    by = {c["name"]: w for c, w in zip(cases, want)}
    assert by["saturated_900_a40"][0] == 32767 and by["pad_slot_q513"][1] == 519 and by["tie_qe_tandem"] == (22, 10, 10) and by["all_zero_q20_t30"] == (0, 23, 29)


def test_300_random_jobs_equal_the_host_form(ctx):
    jobs = Q.random_jobs(300, 600, 123)
    want = [host_form(c) for c in jobs]
    assert run_bytes(ctx, jobs, 1) == want
    assert run_bytes(ctx, jobs[:100], -1) == want[:100]


def test_the_routing_knob_ignores_values_outside_0_to_64():
    gpu.set_ksw_ll_routing(65)
    assert gpu.ksw_ll_reg_max() == Q.REG_MAX_DEFAULT
    gpu.set_ksw_ll_routing(-1)
    assert gpu.ksw_ll_reg_max() == Q.REG_MAX_DEFAULT


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def POS():
    """the named cases of one scoring in position form: their targets in one contig of a small uploaded index, their queries in resident reads (even cases on the
    forward strand, odd ones on the reverse strand). A context of its own: a mapper replaces the resident reads of the context it maps on."""
    ctx = gpu.Context(0, 1 << 30)
    cases = [c for c in Q.make_cases() if (c["a"], c["b"], c["ambi"], c["gapo"], c["gape"]) == (2, 4, 1, 4, 2)]
    made = {}
    tmp = tempfile.mkdtemp()
    idxs = []
    for step in (1, -1):
        reads, ref, jobs = Q.pos_layout(cases, step)
        fa = os.path.join(tmp, "pos%d.fa" % step)
        synth.write_fasta(fa, [ref], prefix="ctg")
        made[step] = (fa, reads, len(ref), jobs)
    yield ctx, cases, made, idxs
    for i in idxs:
        i.close()
    ctx.close()


@pytest.mark.parametrize("reg_max", [Q.REG_MAX_DEFAULT, 32])
@pytest.mark.parametrize("step", [1, -1])
def test_position_form_equals_the_host_form(POS, step, reg_max):
    ctx, cases, made, idxs = POS
    assert len(cases) > 25
    fa, reads, ref_len, layout = made[step]
    idx = gpu.Index(fa, None, k=15, w=50, n_threads=4)
    idxs.append(idx)
    idx.upload(ctx)
    ctx.reads_upload(reads)
    gpu.set_ksw_ll_routing(reg_max)
    jobs = np.zeros(len(cases), gpu.LL_POS_DTYPE)
    lay = np.array(layout, np.int64)
    jobs["qwin_off"], jobs["qwin_len"], jobs["q_pos"], jobs["t_pos"], jobs["step"] = lay[:, 0], lay[:, 1], lay[:, 2], lay[:, 3], step      # (rid 0: the one contig)
    jobs["qlen"], jobs["tlen"] = [len(c["q"]) for c in cases], [len(c["t"]) for c in cases]
    out = ctx.ksw_ll_batch_pos(mat_of(cases[0]), 4, 2, jobs)
    for c, o in zip(cases, out):
        assert tuple(int(v) for v in o) == host_form(c, rev=step < 0), (c["name"], step, reg_max)      # (step -1 reads the stored operands back to front: another job)
    # the refusals of the position form, each naming the job and leaving out as it was
    good = jobs[:1].copy()
    L0, ql0, tl0 = int(good[0]["qwin_len"]), int(good[0]["qlen"]), int(good[0]["tlen"])
    bad_jobs = [dict(rid=1), dict(rid=-1), dict(t_pos=-1), dict(t_pos=ref_len), dict(t_pos=ref_len - tl0 + 1 if step > 0 else tl0 - 2), dict(qwin_off=-1),
                dict(qwin_off=len(reads) - L0 + 1), dict(qwin_len=-1), dict(q_pos=1 << 30), dict(q_pos=-(1 << 30)), dict(qlen=0), dict(tlen=0),
                dict(qlen=gpu.LL_MAX_LEN + 1), dict(step=0), dict(step=2)]
    for ch in bad_jobs:
        two = np.concatenate([good, good])
        for k, v in ch.items():
            two[1][k] = v
        keep = np.full((2, 3), -7, np.int32)
        with pytest.raises(gpu.WmError, match="job 1"):
            ctx.ksw_ll_batch_pos(mat_of(cases[0]), 4, 2, two, out=keep)
        assert (keep == -7).all(), ch
    # a query far outside two-strand space is N, not an error
    far = good.copy(); far[0]["q_pos"] = 5 * L0
    assert int(ctx.ksw_ll_batch_pos(Q.simple_mat(2, 4, 0), 4, 2, far)[0][0]) == 0


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_out_untouched(ctx):
    c = Q.make_cases()[5]
    q_off, t_off, ql, tl, st, seqs = Q.pack([c, c], 1)
    jobs = np.zeros(2, gpu.LL_JOB_DTYPE)
    jobs["q_off"], jobs["t_off"], jobs["qlen"], jobs["tlen"], jobs["step"] = q_off, t_off, ql, tl, st
    m = mat_of(c)
    want = host_form(c)
    assert [tuple(int(v) for v in o) for o in ctx.ksw_ll_batch(m, 4, 2, jobs, seqs)] == [want, want]

    def refused(match, gapo=4, gape=2, **change):
        j = jobs.copy()
        for k, v in change.items():
            j[1][k] = v
        keep = np.full((2, 3), -7, np.int32)
        with pytest.raises(gpu.WmError, match=match):
            ctx.ksw_ll_batch(m, gapo, gape, j, seqs, out=keep)
        assert (keep == -7).all(), (match, change)
    refused("gapo", gapo=0); refused("gapo", gapo=-1); refused("gape", gape=0); refused("int16", gapo=32000, gape=768)
    refused("job 1", qlen=0); refused("job 1", tlen=0); refused("job 1", qlen=-5)
    refused("job 1.*WM_LL_MAX_LEN", qlen=gpu.LL_MAX_LEN + 1); refused("job 1.*WM_LL_MAX_LEN", tlen=gpu.LL_MAX_LEN + 1)
    refused("job 1", step=0); refused("job 1", step=-2)
    refused("job 1", q_off=len(seqs) - int(ql[1]) + 1); refused("job 1", t_off=len(seqs)); refused("job 1", t_off=0xffffffff)
    # gapo + gape = 32767 is the last pair that fits; codes above 4 count as 4
    assert len(ctx.ksw_ll_batch(m, 32000, 767, jobs, seqs)) == 2
    hi = seqs.copy(); hi[hi == 3] = 9
    c4 = Q.case("n", np.where(c["q"] == 3, 4, c["q"]), np.where(c["t"] == 3, 4, c["t"]))
    assert tuple(int(v) for v in ctx.ksw_ll_batch(m, 4, 2, jobs[:1], hi)[0]) == host_form(c4)
    # a position job without an uploaded index or reads (this context has neither)
    pj = np.zeros(1, gpu.LL_POS_DTYPE)
    pj["qwin_len"], pj["qlen"], pj["tlen"], pj["step"] = 10, 5, 5, 1
    keep = np.full((1, 3), -7, np.int32)
    with pytest.raises(gpu.WmError, match="wm_index_upload|wm_reads_upload"):
        ctx.ksw_ll_batch_pos(m, 4, 2, pj, out=keep)
    assert (keep == -7).all()
    assert len(ctx.ksw_ll_batch(m, 4, 2, jobs[:0], seqs)) == 0


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------
def inversion_input(tmp):
    """the reads of tests/test_fix_host.py::test_an_inversion_test_fixes_its_two_neighbours_on_the_host_first"""
    rng = np.random.default_rng(17)
    ref = synth.make_reference(1, 120000, 23, repeat_frac=0.0)
    fa = os.path.join(tmp, "inv.fa")
    synth.write_fasta(fa, ref)
    reads = []
    for i in range(6):
        p = int(rng.integers(2000, 90000))
        r = ref[0][p:p + 9000].copy()
        a = int(rng.integers(3000, 4000)); ln = int(rng.integers(600, 1500))
        r[a:a + ln] = synth.revcomp_codes(r[a:a + ln])
        for q in rng.integers(0, len(r), 90):
            r[q] = (r[q] + 1) % 4
        reads.append(synth.codes_to_ascii(r))
    return "map-ont", fa, 15, 50, reads


def splice_input(tmp):
    """the splice set of tests/test_ll_host.py (k = 9: the end filter asks for scores)"""
    ref = synth.make_reference(2, 200000, 191, repeat_frac=0.05)
    reads = [synth.codes_to_ascii(r) for r in synth.make_transcripts(ref, 16, 192)]
    fa = os.path.join(tmp, "splice.fa")
    synth.write_fasta(fa, ref)
    return "splice", fa, 9, 25, reads


def host_mapper(preset, fa, k, w, reads):
    """the host mapper over the oracle's operations (tests/host_harness), switch off"""
    H = C.CDLL(build.build_harness())
    H.h_index_build.restype = C.c_void_p
    H.h_index_build.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    H.h_map_many.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int, C.POINTER(C.c_char_p), W.i32p, C.c_int, W.i32p, C.c_int, C.POINTER(C.c_int64), W.u32p, C.c_int64, C.POINTER(C.c_int64)]
    H.wm_set_ll_device.argtypes = [C.c_int]
    H.wm_set_ll_device(0)
    hh = H.h_index_build(fa.encode(), b"", k, w, 4)
    n = len(reads)
    ho = np.zeros(16 * 1024, np.int32); co = np.zeros(4000000, np.uint32); hf = (C.c_int64 * (n + 1))(); nc = C.c_int64()
    nh = H.h_map_many(hh, preset.encode(), 0x4 | 0x20, n, (C.c_char_p * n)(*reads), np.array([len(r) for r in reads], np.int32), 2, ho, 1024, hf, co, len(co), C.byref(nc))
    assert nh > 0
    return ho[:16 * nh].reshape(-1, 16).copy(), co[:nc.value].copy(), np.array(list(hf), np.int64)


def reference_mapper(preset, fa, k, w, reads):
    """the goldens' generator (tests/golden/make_golden.py): the real reference through oracle/_ref"""
    R = W.ref()
    R.refshim_idx_build_flag.restype = C.c_void_p
    R.refshim_idx_build_flag.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
    mi = R.refshim_idx_build_flag(fa.encode(), b"", k, w, 0, 4)
    opt = R.refshim_mapopt(preset.encode(), 0x4 | 0x20, mi)
    hits, cigs, first = [], [], [0]
    for i, s in enumerate(reads):
        h = np.zeros(16 * 256, np.int32); c = np.zeros(2000000, np.uint32); nc = C.c_int64()
        n = R.refshim_map(mi, opt, s, len(s), ("read%d" % i).encode(), h, 256, c, len(c), C.byref(nc))
        hits.append(h[:16 * n].reshape(-1, 16).copy()); cigs.append(c[:nc.value].copy()); first.append(first[-1] + n)
    return np.concatenate(hits), np.concatenate(cigs), np.array(first, np.int64)


@pytest.mark.parametrize("make", [inversion_input, splice_input])
def test_mapper_with_the_jobs_on_the_device_gives_the_same_hits_cigars_and_text(ctx, make):
    tmp = tempfile.mkdtemp()
    preset, fa, k, w, reads = make(tmp)
    idx = gpu.Index(fa, None, k=k, w=w, n_threads=8)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, preset, gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG)
    names = ["read%d" % i for i in range(len(reads))]
    try:
        gpu.set_ll_device(0)
        gpu.ll_stats(reset=True)
        text0, hits0, cigars0, first0 = m.map(names, reads)
        assert not any(gpu.ll_stats().values())
        gpu.set_ll_device(1)
        assert gpu.ll_device_enabled()
        text1, hits1, cigars1, first1 = m.map(names, reads)
        st = gpu.ll_stats()
    finally:
        m.close()
        idx.close()
    assert text1 == text0 and np.array_equal(hits1, hits0) and np.array_equal(cigars1, cigars0) and np.array_equal(first1, first0)
    # every read of a wm_map_reads call is resident and no job of these inputs exceeds WM_LL_MAX_LEN: the device served every one
    assert st["deferred"] > 0 and st["on_device"] == st["deferred"] and st["on_host"] == 0 and st["calls"] > 0 and st["cells"] > 0, st
    hh, hc, hf = host_mapper(preset, fa, k, w, reads)
    assert np.array_equal(hh, hits1) and np.array_equal(hc, cigars1) and np.array_equal(hf, first1)
    if W.have_ref():
        rh, rc, rf = reference_mapper(preset, fa, k, w, reads)
        g, h = rh.copy(), hits1.copy()
        for i, s in enumerate(reads):
            E.mask_mapq(len(s), g[int(rf[i]):int(rf[i + 1])], h[int(first1[i]):int(first1[i + 1])], splice=preset == "splice")
        assert np.array_equal(rf, first1) and np.array_equal(g, h) and np.array_equal(rc, cigars1)


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------
def test_two_mapping_calls_in_flight_with_8_host_threads_give_the_same_with_the_switch_on_and_off(ctx):
    tmp = tempfile.mkdtemp()
    preset, fa, k, w, reads = inversion_input(tmp)
    reads = reads[:4]
    idx = gpu.Index(fa, None, k=k, w=w, n_threads=8)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, preset, gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG | gpu.MM_F_OUT_CS)
    m.set_threads(8, 1 << 30)
    halves = [(["a%d" % i for i in range(len(reads))], reads), (["b%d" % i for i in range(len(reads))], reads[::-1])]

    def both_slots():
        with ThreadPoolExecutor(2) as ex:
            fs = [ex.submit(m.map, halves[s][0], halves[s][1], True, s) for s in (0, 1)]
            return [f.result()[0] for f in fs]
    try:
        gpu.set_ll_device(0)
        off = both_slots()
        gpu.set_ll_device(1)
        gpu.ll_stats(reset=True)
        on = both_slots()
        st = gpu.ll_stats()
    finally:
        m.close()
        idx.close()
    assert on == off and all(t.count(b"\n") >= len(reads) for t in on)
    assert st["on_device"] == st["deferred"] > 0 and st["on_host"] == 0 and st["calls"] >= 2, st

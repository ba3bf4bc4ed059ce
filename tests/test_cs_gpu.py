"""GPU: the bodies of the cs:Z / MD:Z tags on the device (csrc/cs_kernel.h behind wm_cs_batch / wm_cs_batch_pos; write_cs_core / write_MD_core,
src/format.c:141-218) — every named case in the three modes under both classes and both tile sizes against the Python restatement of the rules
(cscases.restated; tests/test_cs_emu.py holds it equal to the specification on these very cases), the position form over uploaded reads and a small uploaded
index, the capacity rule, the refusals; and the mapper under --cs / --cs=long / --MD with the bodies produced on the device (wm_set_cs_device), which must print
the very text it prints with the switch off — also with two mapping calls in flight, and through the bound command line against the reference's."""
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import e2e_common as E
import extracases as X
import cscases as Q
from winnowmap_amd import gpu, synth, parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_ref")
WM_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_wm")
ALL_SHORT, ALL_LONG = 1 << 30, 1
DEFAULT_ROUTING = (32768, Q.T)
ROUTES = [(ALL_SHORT, 64), (ALL_SHORT, Q.T), (ALL_LONG, 64), (ALL_LONG, Q.T), DEFAULT_ROUTING]
MODE_FLAGS = {Q.SHORT: gpu.MM_F_OUT_CS, Q.LONG: gpu.MM_F_OUT_CS | gpu.MM_F_OUT_CS_LONG, Q.MD: gpu.MM_F_OUT_MD}


@pytest.fixture(scope="module")
def ctx():
    c = gpu.Context(0, 4 << 30)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def restore_switches_and_routing():
    """all process-global: every test leaves the library's defaults behind"""
    assert gpu.extra_tile_cols() == Q.T and (gpu.CS_SHORT, gpu.CS_LONG, gpu.CS_MD) == Q.MODES
    try:
        yield
    finally:
        gpu.set_extra_routing(*DEFAULT_ROUTING)
        gpu.set_cs_device(-1); gpu.set_eqx_device(-1); gpu.set_fix_device(-1); gpu.set_extra_device(-1)


def pack(cases):
    jobs = np.zeros(len(cases), gpu.EXTRA_JOB_DTYPE)
    seqs, cigs = [], [np.zeros(0, np.uint32)]
    at = ops = 0
    for i, (_, cig, q, t) in enumerate(cases):
        jobs[i] = (at, at + len(q), ops, len(cig))
        seqs += [q, t]; at += len(q) + len(t); cigs.append(cig); ops += len(cig)
    return jobs, np.concatenate(seqs), np.concatenate(cigs).astype(np.uint32)


def check(names, wants, text, res, tag):
    at = 0
    for name, want, r in zip(names, wants, res):
        off, n = int(r["off"]), int(r["len"])
        assert off == at and int(r["pad"]) == 0, (name, tag, off, at)                      # back to back in job order
        got = text[off:off + n].tobytes()
        assert got == want, (name, tag, got[:200], want[:200])                              # byte for byte
        at += n
    assert len(text) == at


@pytest.fixture(scope="module")
def EXPECTED():
    """computed once: every byte-form case with what the restated rules give in the three modes"""
    cases = Q.make_cases() + Q.batch70() + [Q.long_40k()]
    return cases, [[Q.restated(m, c[1], c[2], c[3]) for c in cases] for m in Q.MODES], pack(cases)


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_every_named_case_equals_the_restated_rules(ctx, EXPECTED, long_min, tile, mode):
    gpu.set_extra_routing(long_min, tile)
    assert gpu.extra_tile_cols() == tile
    cases, wants, (jobs, seqs, cigs) = EXPECTED
    assert len(cases) > 140
    text, res = ctx.cs_batch(mode, jobs, seqs, cigs)
    check([c[0] for c in cases], wants[mode], text, res, (mode, long_min, tile))


@pytest.mark.parametrize("mode", Q.MODES)
def test_a_pool_one_byte_too_small_reports_the_needed_size_then_the_exact_size_succeeds(ctx, EXPECTED, mode):
    cases, wants, _ = EXPECTED
    pick = [i for i, c in enumerate(cases) if c[0].startswith("cs_batch70")]
    cases, wants = [cases[i] for i in pick], [wants[mode][i] for i in pick]
    jobs, seqs, cigs = pack(cases)
    needed = sum(len(w) for w in wants)
    with pytest.raises(gpu.WmError) as ei:
        ctx.cs_batch(mode, jobs, seqs, cigs, out_cap=needed - 1)
    assert ei.value.rc == -3 and ei.value.needed == needed
    assert [int(r["len"]) for r in ei.value.res] == [len(w) for w in wants]                # out[] is already filled
    text, res = ctx.cs_batch(mode, jobs, seqs, cigs, out_cap=needed)
    check([c[0] for c in cases], wants, text, res, "exact capacity")


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def POS():
    """extracases' position cases: their contigs as a small uploaded index, their read resident behind a lead. A context of its own: a mapper replaces the
    resident reads of the context it maps on."""
    ctx = gpu.Context(0, 1 << 30)
    P = X.make_pos_cases()
    tmp = tempfile.mkdtemp()
    fa = os.path.join(tmp, "pos.fa")
    synth.write_fasta(fa, [p[4] for p in P], prefix="ctg")
    idx = gpu.Index(fa, None, k=15, w=50, n_threads=4)
    idx.upload(ctx)
    lead = 37
    read = P[0][2]
    assert all(p[2] is read for p in P)
    ctx.reads_upload(np.concatenate([np.full(lead, 4, np.uint8), read, np.full(11, 4, np.uint8)]))
    want = [[] for _ in Q.MODES]
    for name, cig, rd, q_pos, contig, t_pos, score in P:
        ql = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 1)); tl = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 2, 3))
        q = X.two_strand(rd, q_pos, ql); t = contig[t_pos:t_pos + tl]
        for m in Q.MODES:
            want[m].append(Q.restated(m, cig, q, t))
    yield ctx, P, lead, want
    idx.close()
    ctx.close()


@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_position_form_equals_the_restated_rules(POS, long_min, tile, mode):
    ctx, P, lead, want = POS
    gpu.set_extra_routing(long_min, tile)
    jobs = np.zeros(len(P), gpu.EXTRA_POS_DTYPE)
    cigs, ops = [], 0
    for rid, p in enumerate(P):
        jobs[rid] = (lead, len(p[2]), p[3], rid, p[5], ops, len(p[1]))
        cigs.append(p[1]); ops += len(p[1])
    text, res = ctx.cs_batch_pos(mode, jobs, np.concatenate(cigs))
    check([p[0] for p in P], want[mode], text, res, (mode, long_min, tile))
    assert b"N" in text.tobytes() or b"n" in text.tobytes()


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_job(ctx, POS):
    cig, q, t = X.build([(X.M, 100)], seed=1, mm=[40])
    seqs = np.concatenate([q, t])
    two = np.zeros(2, gpu.EXTRA_JOB_DTYPE)
    two[0] = (0, len(q), 0, 1); two[1] = (0, len(q), 0, 1)
    text, res = ctx.cs_batch(Q.SHORT, two, seqs, cig)
    body = Q.restated(Q.SHORT, cig, q, t)
    assert text.tobytes() == body * 2 and body.startswith(b":40*") and body.endswith(b":59")
    # a bad mode
    for mode in (-1, 3):
        with pytest.raises(gpu.WmError, match="mode"):
            ctx.cs_batch(mode, two, seqs, cig)
    # a CIGAR that consumes more query / target than seqs holds behind the offsets — also through ops 7 / 8, which consume both
    bad = two.copy(); bad[1] = (len(seqs) - 99, len(q), 0, 1)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.cs_batch(Q.SHORT, bad, seqs, cig)
    bad = two.copy(); bad[1] = (0, len(seqs) - 99, 0, 1)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.cs_batch(Q.MD, bad, seqs, cig)
    for code in (7, 8):
        with pytest.raises(gpu.WmError, match="job 1"):
            ctx.cs_batch(Q.MD, bad, seqs, np.array([100 << 4 | code], np.uint32))
    # ops beyond n_ops, a negative count
    bad = two.copy(); bad[1] = (0, len(q), 1, 1)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.cs_batch(Q.LONG, bad, seqs, cig)
    bad = two.copy(); bad[0] = (0, len(q), 0, -1)
    with pytest.raises(gpu.WmError, match="job 0"):
        ctx.cs_batch(Q.LONG, bad, seqs, cig)
    # an op code outside {0, 1, 2, 3, 7, 8}, in every mode
    three = np.array([50 << 4, 50 << 4, 3 << 4 | 4, 47 << 4], np.uint32)
    jobs = np.zeros(2, gpu.EXTRA_JOB_DTYPE); jobs[0] = (0, len(q), 0, 1); jobs[1] = (0, len(q), 1, 3)
    for mode in Q.MODES:
        with pytest.raises(gpu.WmError, match="job 1: op 1 has code 4"):
            ctx.cs_batch(mode, jobs, seqs, three)
    # an N op shorter than 2: refused in the cs modes, fine in MD
    three[2] = 1 << 4 | 3
    for mode in (Q.SHORT, Q.LONG):
        with pytest.raises(gpu.WmError, match="job 1: op 1 is an N of length 1"):
            ctx.cs_batch(mode, jobs, seqs, three)
    text, res = ctx.cs_batch(Q.MD, jobs, seqs, three)
    assert int(res[1]["len"]) > 0
    # a job whose bound of output bytes reaches 2^31 (3 bytes per M column): refused before anything is read
    huge = np.array([(0xfffffff << 4)] * 3, np.uint32)
    hj = np.zeros(2, gpu.EXTRA_JOB_DTYPE); hj[0] = (0, len(q), 0, 0); hj[1] = (0, len(q), 0, 3)
    with pytest.raises(gpu.WmError, match="job 1.*2\\^31"):
        ctx.cs_batch(Q.SHORT, hj, seqs, huge)
    # n_cigar == 0 is valid and gives len 0, whatever the offsets say
    z = np.array([(4000000000, 4000000000, 0, 0)], gpu.EXTRA_JOB_DTYPE)
    for mode in Q.MODES:
        text, res = ctx.cs_batch(mode, z, seqs, cig)
        assert len(text) == 0 and int(res[0]["len"]) == 0
    # position form: the target past its contig's end, a contig that does not exist, the (sub)read outside the resident reads, a query far outside two-strand space
    pctx, P, lead, _ = POS
    last = len(P) - 1
    clen, L = len(P[last][4]), len(P[0][2])
    m100 = np.array([100 << 4], np.uint32)
    good = (lead, L, 0, last, clen - 100, 0, 1)
    text, res = pctx.cs_batch_pos(Q.LONG, np.array([good], gpu.EXTRA_POS_DTYPE), m100)
    assert sum(1 for c in text.tobytes() if c in b"ACGTN") + text.tobytes().count(b"*") == 100
    for j in ((lead, L, 0, last, clen - 99, 0, 1), (lead, L, 0, len(P), 0, 0, 1), (lead, L, 0, last, -1, 0, 1), (lead + 12, L, 0, last, 0, 0, 1), (-1, L, 0, last, 0, 0, 1),
              (lead, L, 2 * L, last, 0, 0, 1), (lead, L, -100, last, 0, 0, 1)):
        with pytest.raises(gpu.WmError, match="job 1"):
            pctx.cs_batch_pos(Q.SHORT, np.array([good, j], gpu.EXTRA_POS_DTYPE), m100)


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def GOLDEN(ctx):
    """one index and one mapper per golden, built once and shared by the three modes"""
    made = {}

    def get(name):
        if name not in made:
            tmp = tempfile.mkdtemp()
            preset, fa, kf, k, reads = E.make_golden.inputs(name, tmp)
            idx = gpu.Index(fa, kf, k=k, w=50, n_threads=8)
            idx.upload(ctx)
            made[name] = (idx, preset, reads)
        return made[name]
    yield get
    for idx, _, _ in made.values():
        idx.close()


@pytest.mark.parametrize("mode", Q.MODES)
@pytest.mark.parametrize("name", ["ont_short", "hifi", "asm20"])
def test_mapper_with_the_bodies_from_the_device_prints_the_same_text(ctx, GOLDEN, name, mode):
    idx, preset, reads = GOLDEN(name)
    m = gpu.Mapper(ctx, idx, preset, gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG | MODE_FLAGS[mode])
    names = ["read%d" % i for i in range(len(reads))]
    try:
        gpu.set_cs_device(0)
        gpu.cs_stats(reset=True)
        text0, hits0, cigars0, first0 = m.map(names, reads)
        assert not any(gpu.cs_stats().values())
        gpu.set_cs_device(1)
        assert gpu.cs_device_enabled()
        text1, hits1, cigars1, first1 = m.map(names, reads)
        st = gpu.cs_stats()
    finally:
        m.close()
    tag = b"\tMD:Z:" if mode == Q.MD else b"\tcs:Z:"
    assert text1 == text0 and text1.count(tag) > 0
    assert np.array_equal(hits1, hits0) and np.array_equal(cigars1, cigars0) and np.array_equal(first1, first0)      # hits and CIGARs are untouched
    E.compare(name, hits1, cigars1, first1, reads)
    # every read of a wm_map_reads call is resident: every deferred region was served on the device
    assert st["deferred"] == text1.count(tag) and st["on_device"] == st["deferred"] and st["on_host"] == 0 and st["calls"] > 0 and st["bytes"] > 0, st


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------
def test_two_mapping_calls_in_flight_with_8_host_threads_give_the_same_with_the_switch_on_and_off(ctx):
    tmp = tempfile.mkdtemp()
    preset, fa, kf, k, reads = E.make_golden.inputs("ont", tmp)
    reads = reads[:12]
    idx = gpu.Index(fa, kf, k=k, w=50, n_threads=8)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, preset, gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG | gpu.MM_F_OUT_CS)
    m.set_threads(8, 1 << 30)
    halves = [(["a%d" % i for i in range(len(reads))], reads), (["b%d" % i for i in range(len(reads))], reads[::-1])]

    def both_slots():
        with ThreadPoolExecutor(2) as ex:
            fs = [ex.submit(m.map, halves[s][0], halves[s][1], True, s) for s in (0, 1)]
            return [f.result()[0] for f in fs]
    try:
        gpu.set_cs_device(0)
        off = both_slots()
        gpu.set_cs_device(1)
        gpu.cs_stats(reset=True)
        on = both_slots()
        st = gpu.cs_stats()
    finally:
        m.close()
        idx.close()
    assert on == off and all(t.count(b"\n") >= len(reads) and b"\tcs:Z:" in t for t in on)
    assert st["on_device"] == st["deferred"] > 0 and st["on_host"] == 0 and st["calls"] >= 2, st


# ---- (f) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.exists(REF_BIN) and os.path.exists(WM_BIN)), reason="oracle/_ref/winnowmap_ref / winnowmap_wm not built")
@pytest.mark.parametrize("fmt,tagopt", [("-cx", "--cs"), ("-ax", "--MD")])
def test_the_bound_cli_with_the_switch_on_prints_what_winnowmap_ref_prints(fmt, tagopt):
    tmp = tempfile.mkdtemp()
    ref = synth.make_reference(2, 300000, 31, repeat_frac=0.08)
    fa = os.path.join(tmp, "ref.fa")
    synth.write_fasta(fa, ref, prefix="chr")
    km, cnt = synth.repetitive_kmers(ref, 15)
    kf = os.path.join(tmp, "rep.txt")
    synth.write_kmer_list(kf, km, cnt, 15)
    reads, _ = synth.make_reads(ref, 16, 12000, 32, profile="ont", sv_frac=0.2)
    reads += synth.make_reads(ref, 8, 3000, 33, profile="ont")[0]
    rq = os.path.join(tmp, "reads.fa")
    with open(rq, "wb") as f:
        for i, r in enumerate(reads):
            f.write(b">r%d\n" % i + synth.codes_to_ascii(r) + b"\n")

    def run(binary, args):
        p = subprocess.run([binary] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, WM_CS_DEV="1", WM_EXTRA_REPORT="1"), timeout=600)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        return p.stdout, p.stderr
    args = ["-t", "4", "-W", kf, tagopt, fmt, "map-ont", fa, rq]
    want, got = run(REF_BIN, args)[0], run(WM_BIN, args)
    d = parity.diff_texts(want, got[0], sam=fmt == "-ax")
    assert d["reads"] >= 20 and d["hits"] >= 20 and d["mismatches"] == 0, (fmt, d)
    tag = b"\tMD:Z:" if tagopt == "--MD" else b"\tcs:Z:"
    assert got[0].count(tag) >= 20 and got[0].count(tag) == want.count(tag)
    assert b"[wm] cs: " in got[1] and b" 0 on the host" in got[1], got[1][-500:]           # the switch was on, and the device served every region (WM_EXTRA_REPORT, host/wm_ops.cpp)

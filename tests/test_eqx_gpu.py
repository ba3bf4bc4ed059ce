"""GPU: mm_update_cigar_eqx on the device (csrc/eqx_kernel.h behind wm_eqx_batch / wm_eqx_batch_pos; src/align.c:169-238) — every named case under both classes
and both tile sizes against the specification (csrc/cigar_eqx.h, through its numpy restatement), the position form over uploaded reads and a small
uploaded index, the capacity rule, the refusals; and the mapper under MM_F_EQX with the rewriting deferred to the device (wm_set_eqx_device), which must give the
very output it gives with the switch off — also with the two sibling switches on, and with two mapping calls in flight."""
import ctypes as C
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import wmtest as W
import e2e_common as E
import extracases as X
import eqxcases as Q
from winnowmap_amd import gpu, synth, parity

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_ref")
WM_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_wm")
ALL_SHORT, ALL_LONG = 1 << 30, 1
ROUTES = [(ALL_SHORT, 64), (ALL_SHORT, Q.T), (ALL_LONG, 64), (ALL_LONG, Q.T)]
DEFAULT_ROUTING = (32768, Q.T)
FLAGS = gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG | gpu.MM_F_EQX


@pytest.fixture(scope="module")
def ctx():
    c = gpu.Context(0, 4 << 30)
    yield c
    c.close()


@pytest.fixture(scope="module")
def SPEC():
    """the specification through its numpy restatement (tests/test_eqx_emu.py holds the two equal on these very cases; the GPU tests load no emulator)"""
    return Q.restated


@pytest.fixture(autouse=True)
def restore_switches_and_routing():
    """all process-global: every test leaves the library's defaults behind"""
    assert gpu.extra_tile_cols() == Q.T
    try:
        yield
    finally:
        gpu.set_extra_routing(*DEFAULT_ROUTING)
        gpu.set_eqx_device(-1); gpu.set_fix_device(-1); gpu.set_extra_device(-1)


def pack(cases):
    jobs = np.zeros(len(cases), gpu.EXTRA_JOB_DTYPE)
    seqs, cigs = [], [np.zeros(0, np.uint32)]
    at = ops = 0
    for i, (_, cig, q, t) in enumerate(cases):
        jobs[i] = (at, at + len(q), ops, len(cig))
        seqs += [q, t]; at += len(q) + len(t); cigs.append(cig); ops += len(cig)
    return jobs, np.concatenate(seqs), np.concatenate(cigs).astype(np.uint32)


def check(cases, wants, pool, res, tag):
    at = 0
    for c, (want, ip), r in zip(cases, wants, res):
        off, n = int(r["off"]), int(r["n_cigar"])
        assert off == at and int(r["in_place"]) == ip, (c[0], tag, off, at, int(r["in_place"]), ip)      # back to back in job order; branch for branch
        assert n == len(want) and np.array_equal(pool[off:off + n], want), (c[0], tag)                   # op for op
        at += n
    assert len(pool) == at


@pytest.fixture(scope="module")
def EXPECTED(SPEC):
    """computed once: every byte-form case with what the specification gives"""
    cases = Q.make_cases() + Q.batch70() + [Q.long_40k()]
    return cases, [SPEC(c[1], c[2], c[3]) for c in cases]


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_min,tile", ROUTES + [DEFAULT_ROUTING])
def test_every_named_case_equals_the_specification(ctx, EXPECTED, long_min, tile):
    gpu.set_extra_routing(long_min, tile)
    assert gpu.extra_tile_cols() == tile
    cases, wants = EXPECTED
    assert len(cases) > 130
    jobs, seqs, cigs = pack(cases)
    pool, res = ctx.eqx_batch(jobs, seqs, cigs)
    check(cases, wants, pool, res, (long_min, tile))


def test_a_pool_one_op_too_small_reports_the_needed_count_then_the_exact_size_succeeds(ctx, EXPECTED):
    cases, wants = EXPECTED
    pick = [i for i, c in enumerate(cases) if c[0].startswith("batch70")]
    cases, wants = [cases[i] for i in pick], [wants[i] for i in pick]
    jobs, seqs, cigs = pack(cases)
    needed = sum(len(w) for w, _ in wants)
    with pytest.raises(gpu.WmError) as ei:
        ctx.eqx_batch(jobs, seqs, cigs, out_cap=needed - 1)
    assert ei.value.rc == -3 and ei.value.needed == needed
    assert [int(r["n_cigar"]) for r in ei.value.res] == [len(w) for w, _ in wants]         # out[] is already filled
    pool, res = ctx.eqx_batch(jobs, seqs, cigs, out_cap=needed)
    check(cases, wants, pool, res, "exact capacity")


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def POS(SPEC):
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
    want = []
    for name, cig, rd, q_pos, contig, t_pos, score in P:
        ql = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 1)); tl = sum(int(w) >> 4 for w in cig if (int(w) & 0xf) in (0, 2, 3))
        q = np.concatenate([X.two_strand(rd, q_pos, ql), np.full(16, 4, np.uint8)]); t = np.concatenate([contig[t_pos:t_pos + tl], np.full(16, 4, np.uint8)])
        want.append(SPEC(cig, q, t))
    yield ctx, P, lead, want
    idx.close()
    ctx.close()


@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_position_form_equals_the_specification(POS, long_min, tile):
    ctx, P, lead, want = POS
    gpu.set_extra_routing(long_min, tile)
    jobs = np.zeros(len(P), gpu.EXTRA_POS_DTYPE)
    cigs, ops = [], 0
    for rid, p in enumerate(P):
        jobs[rid] = (lead, len(p[2]), p[3], rid, p[5], ops, len(p[1]))
        cigs.append(p[1]); ops += len(p[1])
    pool, res = ctx.eqx_batch_pos(jobs, np.concatenate(cigs))
    check([(p[0],) for p in P], want, pool, res, (long_min, tile))
    assert any((int(w) & 0xf) == 8 for w in pool)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_job(ctx, POS):
    cig, q, t = X.build([(X.M, 100)], seed=1, mm=[40])
    seqs = np.concatenate([q, t])
    two = np.zeros(2, gpu.EXTRA_JOB_DTYPE)
    two[0] = (0, len(q), 0, 1); two[1] = (0, len(q), 0, 1)
    pool, res = ctx.eqx_batch(two, seqs, cig)
    assert [int(w) for w in pool] == [40 << 4 | 7, 1 << 4 | 8, 59 << 4 | 7] * 2
    # a CIGAR that consumes more query / target than seqs holds behind the offsets
    bad = two.copy(); bad[1] = (len(seqs) - 99, len(q), 0, 1)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.eqx_batch(bad, seqs, cig)
    bad = two.copy(); bad[1] = (0, len(seqs) - 99, 0, 1)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.eqx_batch(bad, seqs, cig)
    # ops beyond n_ops, a negative count
    bad = two.copy(); bad[1] = (0, len(q), 1, 1)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.eqx_batch(bad, seqs, cig)
    bad = two.copy(); bad[0] = (0, len(q), 0, -1)
    with pytest.raises(gpu.WmError, match="job 0"):
        ctx.eqx_batch(bad, seqs, cig)
    # n_cigar == 0 is valid and gives nothing, whatever the offsets say
    z = np.array([(4000000000, 4000000000, 0, 0)], gpu.EXTRA_JOB_DTYPE)
    pool, res = ctx.eqx_batch(z, seqs, cig)
    assert len(pool) == 0 and int(res[0]["n_cigar"]) == 0
    # position form: the target past its contig's end, a contig that does not exist, the (sub)read outside the resident reads, a query far outside two-strand space
    pctx, P, lead, _ = POS
    last = len(P) - 1
    clen, L = len(P[last][4]), len(P[0][2])
    m100 = np.array([100 << 4], np.uint32)
    good = (lead, L, 0, last, clen - 100, 0, 1)
    pool, res = pctx.eqx_batch_pos(np.array([good], gpu.EXTRA_POS_DTYPE), m100)
    assert sum(int(w) >> 4 for w in pool) == 100
    for j in ((lead, L, 0, last, clen - 99, 0, 1), (lead, L, 0, len(P), 0, 0, 1), (lead, L, 0, last, -1, 0, 1), (lead + 12, L, 0, last, 0, 0, 1), (-1, L, 0, last, 0, 0, 1),
              (lead, L, 2 * L, last, 0, 0, 1), (lead, L, -100, last, 0, 0, 1)):
        with pytest.raises(gpu.WmError, match="job 1"):
            pctx.eqx_batch_pos(np.array([good, j], gpu.EXTRA_POS_DTYPE), m100)


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------
def collapsed(hits, cigars):
    """7 / 8 back to 0 and neighbours merged, per hit -> (hits with the new op counts, cigars)"""
    h = hits.copy()
    out, at = [], 0
    for r in h:
        n = int(r[7])
        ops = []
        for w in cigars[at:at + n]:
            op, ln = int(w) & 0xf, int(w) >> 4
            op = 0 if op in (7, 8) else op
            if ops and ops[-1][0] == op:
                ops[-1][1] += ln
            else:
                ops.append([op, ln])
        at += n
        r[7] = len(ops)
        out += [ln << 4 | op for op, ln in ops]
    assert at == len(cigars)
    return h, np.array(out, np.uint32)


# (alone and with both sibling switches on, on every golden; the two mixed combinations on the smallest one)
@pytest.mark.parametrize("name,fix,extra", [(n, f, f) for n in ("ont_short", "hifi", "asm20") for f in (0, 1)] + [("ont_short", 1, 0), ("ont_short", 0, 1)])
def test_mapper_with_the_rewriting_on_the_device_gives_the_same_as_with_it_off(ctx, name, fix, extra):
    tmp = tempfile.mkdtemp()
    preset, fa, kf, k, reads = E.make_golden.inputs(name, tmp)
    idx = gpu.Index(fa, kf, k=k, w=50, n_threads=8)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, preset, FLAGS)
    names = ["read%d" % i for i in range(len(reads))]
    try:
        gpu.set_fix_device(fix); gpu.set_extra_device(extra)
        gpu.set_eqx_device(0)
        gpu.eqx_stats(reset=True)
        text0, hits0, cigars0, first0 = m.map(names, reads)
        assert not any(gpu.eqx_stats().values())
        gpu.set_eqx_device(1)
        assert gpu.eqx_device_enabled()
        text1, hits1, cigars1, first1 = m.map(names, reads)
        st = gpu.eqx_stats()
    finally:
        m.close()
        idx.close()
    assert text1 == text0 and np.array_equal(hits1, hits0) and np.array_equal(cigars1, cigars0) and np.array_equal(first1, first0)
    assert b"=" in text1 and not ((cigars1 & 0xf) == 0).any() and ((cigars1 & 0xf) == 8).any()
    # collapsed, the CIGARs are the goldens'
    ch, cc = collapsed(hits1, cigars1)
    E.compare(name, ch, cc, first1, reads)
    # every read of a wm_map_reads call is resident: every deferred region was served on the device
    assert st["deferred"] > 0 and st["on_device"] == st["deferred"] and st["on_host"] == 0 and st["calls"] > 0 and st["columns"] > 0, st
    if W.have_ref() and (fix, extra) == (0, 0):
        R = W.ref()
        mi = R.refshim_idx_build(fa.encode(), (kf or "").encode(), k, 50, 4)
        opt = R.refshim_mapopt(preset.encode(), FLAGS, mi)
        at = 0
        for i, s in enumerate(reads):
            rh = np.zeros(16 * 256, np.int32); rc = np.zeros(4000000, np.uint32); rnc = C.c_int64()
            rn = R.refshim_map(mi, opt, s, len(s), ("read%d" % i).encode(), rh, 256, rc, len(rc), C.byref(rnc))
            a = hits1[int(first1[i]):int(first1[i + 1])].copy(); b = rh[:16 * rn].reshape(-1, 16).copy()
            assert len(a) == rn, (name, i)
            E.mask_mapq(len(s), a, b)
            assert np.array_equal(a, b), (name, i)
            assert np.array_equal(cigars1[at:at + rnc.value], rc[:rnc.value]), (name, i)
            at += rnc.value
        assert at == len(cigars1)


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------
def test_two_mapping_calls_in_flight_with_8_host_threads_give_the_same_with_the_switch_on_and_off(ctx):
    tmp = tempfile.mkdtemp()
    preset, fa, kf, k, reads = E.make_golden.inputs("ont", tmp)
    reads = reads[:12]
    idx = gpu.Index(fa, kf, k=k, w=50, n_threads=8)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, preset, FLAGS)
    m.set_threads(8, 1 << 30)
    halves = [(["a%d" % i for i in range(len(reads))], reads), (["b%d" % i for i in range(len(reads))], reads[::-1])]

    def both_slots():
        with ThreadPoolExecutor(2) as ex:
            fs = [ex.submit(m.map, halves[s][0], halves[s][1], True, s) for s in (0, 1)]
            return [f.result()[0] for f in fs]
    try:
        gpu.set_eqx_device(0)
        off = both_slots()
        gpu.set_eqx_device(1)
        gpu.eqx_stats(reset=True)
        on = both_slots()
        st = gpu.eqx_stats()
    finally:
        m.close()
        idx.close()
    assert on == off and all(t.count(b"\n") >= len(reads) and b"=" in t for t in on)
    assert st["on_device"] == st["deferred"] > 0 and st["on_host"] == 0 and st["calls"] >= 2, st


# ---- (f) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.skipif(not (os.path.exists(REF_BIN) and os.path.exists(WM_BIN)), reason="oracle/_ref/winnowmap_ref / winnowmap_wm not built")
@pytest.mark.parametrize("fmt,dev", [("-cx", "0"), ("-ax", "1")])
def test_the_bound_cli_with_eqx_prints_what_winnowmap_ref_eqx_prints(fmt, dev):
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
        p = subprocess.run([binary] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=dict(os.environ, WM_EQX_DEV=dev), timeout=600)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        return p.stdout
    args = ["-t", "4", "-W", kf, "--eqx", fmt, "map-ont", fa, rq]
    want, got = run(REF_BIN, args), run(WM_BIN, args)
    d = parity.diff_texts(want, got, sam=fmt == "-ax")
    assert d["reads"] >= 20 and d["hits"] >= 20 and d["mismatches"] == 0, (fmt, d)
    assert b"=" in got and b"X" in got

"""GPU: mm_fix_cigar on the device, alone and fused with the scan of the final CIGAR (csrc/fix_kernel.h + extra_kernel.h behind wm_fix_extra_batch /
wm_fix_extra_batch_pos; src/align.c:91-167, 240-286) — every named and random case of fixcases against the specification (csrc/cigar_fix.h: CIGAR, count, both
shifts, `changed`) and, fused, against wm_extra_walk on the fixed CIGAR at both routings; the position form over uploaded reads and a small uploaded index; the
refusals; and the mapper with both halves deferred to the device (wm_set_fix_device), which must give the goldens and the very text it gives with the switch off —
also with two mapping calls in flight."""
import ctypes as C
import os
import tempfile
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import wmtest as W
import e2e_common as E
import extracases as X
import fixcases as F
from winnowmap_amd import build, gpu, synth

pytestmark = pytest.mark.gpu

ALL_SHORT, ALL_LONG = 1 << 30, 1
ROUTES = [(ALL_SHORT, X.T), (ALL_LONG, 64)]
DEFAULT_ROUTING = (32768, X.T)
i32p = np.ctypeslib.ndpointer(np.int32, flags="C")


@pytest.fixture(scope="module")
def ctx():
    c = gpu.Context(0, 4 << 30)
    yield c
    c.close()


@pytest.fixture(scope="module")
def SPEC():
    """the specification through its Python restatement (tests/test_fix_emu.py holds the two equal on these very cases; the GPU tests load no emulator)"""
    def spec(cig, q, t):
        fixed, qs, ts, ch, _ = F.fix_py(cig, q, t)
        return np.array(fixed, np.uint32), np.array([len(fixed), qs, ts, ch], np.int32)
    return spec


@pytest.fixture(scope="module")
def WALK():
    L = C.CDLL(build.build_harness())
    L.h_extra_walk_both.argtypes = [C.c_void_p, C.c_void_p, W.u32p, C.c_int] + [C.c_int] * 5 + [i32p, i32p]

    def walk(cig, q, t, sc):
        f, g = np.zeros(6, np.int32), np.zeros(6, np.int32)
        cg = np.ascontiguousarray(cig, np.uint32) if len(cig) else np.zeros(1, np.uint32)
        q = np.ascontiguousarray(q); t = np.ascontiguousarray(t)
        L.h_extra_walk_both(q.ctypes.data, t.ctypes.data, cg, len(cig), *[int(v) for v in sc], f, g)
        return g
    return walk


@pytest.fixture(autouse=True)
def restore_switches_and_routing():
    try:
        yield
    finally:
        gpu.set_extra_routing(*DEFAULT_ROUTING)
        gpu.set_fix_device(-1)
        gpu.set_extra_device(-1)


@pytest.fixture(scope="module")
def EXPECTED(SPEC, WALK):
    """computed once: every byte-form case with the specification's fixed CIGAR and results, and wm_extra_walk over that CIGAR with the operands advanced"""
    out = []
    for c in F.make_cases() + F.batch70() + F.random_cases() + F.random_zero_cases():
        wc, wf = SPEC(c[1], c[2], c[3])
        out.append((c, wc, wf, WALK(wc, c[2][wf[1]:], c[3][wf[2]:], c[4])))
    return out


def run_bytes(ctx, cases, score):
    jobs = np.zeros(len(cases), gpu.EXTRA_JOB_DTYPE)
    seqs, cigs = [], [np.zeros(0, np.uint32)]
    at = ops = 0
    for i, (_, cig, q, t, _) in enumerate(cases):
        jobs[i] = (at, at + len(q), ops, len(cig))
        seqs += [q, t]; at += len(q) + len(t); cigs.append(cig); ops += len(cig)
    out, fix, extra = ctx.fix_extra_batch(score, jobs, np.concatenate(seqs), np.concatenate(cigs).astype(np.uint32))
    return [(out[j["cig_off"]:j["cig_off"] + f[0]], f, None if extra is None else extra[i]) for i, (j, f) in enumerate(zip(jobs, fix))]


def by_score(rows):
    groups = {}
    for r in rows:
        groups.setdefault(tuple(r[0][4]), []).append(r)
    return list(groups.values())


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
def test_every_case_in_byte_form_equals_the_specification(ctx, EXPECTED):
    got = run_bytes(ctx, [r[0] for r in EXPECTED], None)
    for (c, wc, wf, _), (gc, gf, gx) in zip(EXPECTED, got):
        assert np.array_equal(gf, wf) and np.array_equal(gc, wc) and gx is None, (c[0], gf, wf, gc[:12], wc[:12])
    assert len(EXPECTED) > 530


@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_the_fused_form_equals_wm_extra_walk_on_the_fixed_cigar(ctx, EXPECTED, long_min, tile):
    gpu.set_extra_routing(long_min, tile)
    for group in by_score(EXPECTED):
        got = run_bytes(ctx, [r[0] for r in group], group[0][0][4])
        for (c, wc, wf, wx), (gc, gf, gx) in zip(group, got):
            assert np.array_equal(gf, wf) and np.array_equal(gc, wc), (c[0], gf, wf)
            assert np.array_equal(gx, wx), (c[0], long_min, tile, gx, wx)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def POS(SPEC, WALK):
    """the position cases: their contigs as a small uploaded index, their read resident behind a lead. A context of its own: a mapper replaces the resident reads
    of the context it maps on."""
    ctx = gpu.Context(0, 1 << 30)
    P = F.make_pos_cases()
    tmp = tempfile.mkdtemp()
    fa = os.path.join(tmp, "pos.fa")
    synth.write_fasta(fa, [p[4] for p in P], prefix="ctg")
    idx = gpu.Index(fa, None, k=15, w=50, n_threads=4)
    idx.upload(ctx)
    read = P[0][2]
    assert all(p[2] is read for p in P)
    ctx.reads_upload(np.concatenate([np.full(F.LEAD, 4, np.uint8), read, np.full(11, 4, np.uint8)]))
    want = []
    for p in P:
        q, t = F.pos_operands(p)
        wc, wf = SPEC(p[1], q, t)
        want.append((wc, wf, WALK(wc, q[wf[1]:], t[wf[2]:], p[6])))
    yield ctx, P, want
    idx.close()
    ctx.close()


@pytest.mark.parametrize("long_min,tile,fused", [(ALL_SHORT, X.T, False), (ALL_SHORT, X.T, True), (ALL_LONG, 64, True)])
def test_position_form_equals_the_specification(POS, long_min, tile, fused):
    ctx, P, want = POS
    gpu.set_extra_routing(long_min, tile)
    for score in sorted(set(tuple(p[6]) for p in P)):
        G = [(rid, p) for rid, p in enumerate(P) if tuple(p[6]) == score]
        jobs = np.zeros(len(G), gpu.EXTRA_POS_DTYPE)
        cigs, ops = [], 0
        for i, (rid, p) in enumerate(G):
            jobs[i] = (F.LEAD, len(p[2]), p[3], rid, p[5], ops, len(p[1]))
            cigs.append(p[1]); ops += len(p[1])
        out, fix, extra = ctx.fix_extra_batch_pos(score if fused else None, jobs, np.concatenate(cigs))
        for i, (rid, p) in enumerate(G):
            wc, wf, wx = want[rid]
            o = int(jobs[i]["cig_off"])
            assert np.array_equal(fix[i], wf) and np.array_equal(out[o:o + fix[i][0]], wc), (p[0], fix[i], wf)
            if fused:
                assert np.array_equal(extra[i], wx), (p[0], long_min, tile, extra[i], wx)


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_job(ctx, POS):
    cig, q, t = X.build([(X.M, 50), (X.I, 2), (X.M, 48)], seed=1)
    seqs = np.concatenate([q, t])
    two = np.zeros(2, gpu.EXTRA_JOB_DTYPE)
    two[0] = (0, len(q), 0, 3); two[1] = (0, len(q), 0, 3)
    out, fix, extra = ctx.fix_extra_batch(X.ONT, two, seqs, cig)
    assert fix[1][0] == 3 and extra[1][4] == 100 and extra[1][5] == 98
    # a zero-length op of code >= 3 (the reference indexes s[op] out of bounds there)
    for bad_op in (3, 4, 9):
        both = np.concatenate([cig, np.array([50 << 4, 0 << 4 | bad_op, 50 << 4], np.uint32)])
        bad = two.copy(); bad[1] = (0, len(q), 3, 3)
        with pytest.raises(gpu.WmError, match="job 1.*length 0"):
            ctx.fix_extra_batch(X.ONT, bad, seqs, both)
        with pytest.raises(gpu.WmError, match="job 1.*length 0"):
            ctx.fix_extra_batch(None, bad, seqs, both)
    # lengths that add up to 2^31 or more (the merge sweep's ordered scans are int32): nine N ops of 2^28 - 1 bases
    huge = np.concatenate([cig, np.array([10 << 4] + [((1 << 28) - 1) << 4 | 3] * 9 + [10 << 4], np.uint32)])
    bad = two.copy(); bad[1] = (0, len(q), 3, 11)
    with pytest.raises(gpu.WmError, match=r"job 1.*add up to 2\^31"):
        ctx.fix_extra_batch(None, bad, seqs, huge)
    with pytest.raises(gpu.WmError, match=r"job 1.*add up to 2\^31"):
        ctx.fix_extra_batch(X.ONT, bad, seqs, huge)
    # ops beyond n_ops
    bad = two.copy(); bad[1] = (0, len(q), 1, 3)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.fix_extra_batch(X.ONT, bad, seqs, cig)
    bad = two.copy(); bad[0] = (0, len(q), 0, -1)
    with pytest.raises(gpu.WmError, match="job 0"):
        ctx.fix_extra_batch(None, bad, seqs, cig)
    # a CIGAR that consumes more than is held
    bad = two.copy(); bad[1] = (len(seqs) - 99, len(q), 0, 3)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.fix_extra_batch(X.ONT, bad, seqs, cig)
    bad = two.copy(); bad[1] = (0, len(seqs) - 97, 0, 3)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.fix_extra_batch(None, bad, seqs, cig)
    # the WM_EXTRA_MAX_ABS limit, on the RAW CIGAR: 98 M columns * match + (q + 2 e)
    big = (gpu.EXTRA_MAX_ABS - 8) // 98
    out, fix, extra = ctx.fix_extra_batch((big, -4, -1, 4, 2), two, seqs, cig)
    assert fix[0][0] in (1, 3)
    with pytest.raises(gpu.WmError, match="job 0.*WM_EXTRA_MAX_ABS"):
        ctx.fix_extra_batch((big + 1, -4, -1, 4, 2), two, seqs, cig)
    # score and extra_out go together (the binding always pairs them); n_cigar == 0 is valid and gives zeros, whatever the offsets say
    z = np.array([(4000000000, 4000000000, 0, 0)], gpu.EXTRA_JOB_DTYPE)
    out, fix, extra = ctx.fix_extra_batch(X.ONT, z, seqs, cig)
    assert not fix.any() and not extra.any()
    out, fix, extra = ctx.fix_extra_batch(None, z, seqs, cig)
    assert not fix.any() and extra is None
    # position form: the target past its contig's end, a contig that does not exist, the (sub)read outside the resident reads
    pctx, P, _ = POS
    last = len(P) - 1
    clen, L = len(P[last][4]), len(P[0][2])
    m100 = np.array([60 << 4, 2 << 4 | 1, 38 << 4], np.uint32)
    good = (F.LEAD, L, 0, last, clen - 98, 0, 3)
    out, fix, extra = pctx.fix_extra_batch_pos(X.ONT, np.array([good], gpu.EXTRA_POS_DTYPE), m100)
    assert extra[0][5] == 98
    for j in ((F.LEAD, L, 0, last, clen - 97, 0, 3), (F.LEAD, L, 0, len(P), 0, 0, 3), (F.LEAD, L, 0, last, -1, 0, 3), (F.LEAD + 12, L, 0, last, 0, 0, 3), (-1, L, 0, last, 0, 0, 3),
              (F.LEAD, L, 2 * L, last, 0, 0, 3), (F.LEAD, L, -100, last, 0, 0, 3)):
        with pytest.raises(gpu.WmError, match="job 1"):
            pctx.fix_extra_batch_pos(X.ONT, np.array([good, j], gpu.EXTRA_POS_DTYPE), m100)
    with pytest.raises(gpu.WmError, match="job 1.*length 0"):
        pctx.fix_extra_batch_pos(None, np.array([good, (F.LEAD, L, 0, last, 0, 3, 1)], gpu.EXTRA_POS_DTYPE), np.concatenate([m100, np.array([3], np.uint32)]))


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ont_short", "hifi", "asm20"])
def test_mapper_with_both_halves_on_the_device_gives_the_golden_and_the_same_text(ctx, name):
    tmp = tempfile.mkdtemp()
    preset, fa, kf, k, reads = E.make_golden.inputs(name, tmp)
    idx = gpu.Index(fa, kf, k=k, w=50, n_threads=8)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, preset, gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG)
    names = ["read%d" % i for i in range(len(reads))]
    try:
        gpu.set_fix_device(0)
        gpu.fix_stats(reset=True); gpu.extra_stats(reset=True)
        text0, hits0, cigars0, first0 = m.map(names, reads)
        assert gpu.fix_stats()["deferred"] == 0 and gpu.extra_stats()["deferred"] == 0
        gpu.set_fix_device(1)
        assert gpu.fix_device_enabled()
        text1, hits1, cigars1, first1 = m.map(names, reads)
        st = gpu.fix_stats(); xs = gpu.extra_stats()
    finally:
        m.close()
        idx.close()
    E.compare(name, hits1, cigars1, first1, reads)
    assert text1 == text0 and np.array_equal(hits1, hits0) and np.array_equal(cigars1, cigars0)
    # every read of a wm_map_reads call is resident: no region may be fixed by the host form of the batched request; the only host fixes are the neighbours of an
    # inversion test, and their scans still run on the device
    assert st["deferred"] > 0 and st["on_host"] == 0 and st["on_device"] + st["early_on_host"] == st["deferred"] and st["calls"] > 0 and st["columns"] > 0, st
    assert xs["deferred"] == xs["on_device"] == st["early_on_host"] and xs["on_host"] == 0 and (xs["columns"] > 0) == (st["early_on_host"] > 0), (st, xs)


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------
def test_two_mapping_calls_in_flight_with_8_host_threads_give_the_same_with_the_switch_on_and_off(ctx):
    tmp = tempfile.mkdtemp()
    preset, fa, kf, k, reads = E.make_golden.inputs("ont", tmp)
    reads = reads[:12]
    idx = gpu.Index(fa, kf, k=k, w=50, n_threads=8)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, preset, gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG)
    m.set_threads(8, 1 << 30)
    halves = [(["a%d" % i for i in range(len(reads))], reads), (["b%d" % i for i in range(len(reads))], reads[::-1])]

    def both_slots():
        with ThreadPoolExecutor(2) as ex:
            fs = [ex.submit(m.map, halves[s][0], halves[s][1], True, s) for s in (0, 1)]
            return [f.result()[0] for f in fs]
    try:
        gpu.set_fix_device(0)
        off = both_slots()
        gpu.set_fix_device(1)
        gpu.fix_stats(reset=True)
        on = both_slots()
        st = gpu.fix_stats()
    finally:
        m.close()
        idx.close()
    assert on == off and all(t.count(b"\n") >= len(reads) for t in on)
    assert st["on_device"] + st["early_on_host"] == st["deferred"] > 0 and st["on_host"] == 0 and st["calls"] >= 2, st

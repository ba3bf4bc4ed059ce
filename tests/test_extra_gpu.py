"""GPU: the scan of mm_update_extra over final CIGARs on the device (csrc/extra_kernel.h behind wm_extra_batch / wm_extra_batch_pos; src/align.c:240-286) —
every named case under both classes and both tile sizes against wm_extra_walk (the harness's generic walk) and, where oracle/_ref is built, the reference's own
mm_update_extra; the position form over uploaded reads and a small uploaded index; the refusals; and the mapper with the scans deferred to the device
(wm_set_extra_device), which must give the goldens and the very text it gives with the switch off — also with two mapping calls in flight."""
import ctypes as C
import os
import tempfile
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import wmtest as W
import e2e_common as E
import extracases as X
from winnowmap_amd import build, gpu, synth

pytestmark = pytest.mark.gpu

ALL_SHORT, ALL_LONG = 1 << 30, 1
ROUTES = [(ALL_SHORT, 64), (ALL_SHORT, X.T), (ALL_LONG, 64), (ALL_LONG, X.T)]
DEFAULT_ROUTING = (32768, X.T)


@pytest.fixture(scope="module")
def ctx():
    c = gpu.Context(0, 4 << 30)
    yield c
    c.close()


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(build.build_harness())
    i32p = np.ctypeslib.ndpointer(np.int32, flags="C")
    L.h_extra_walk_both.argtypes = [C.c_void_p, C.c_void_p, W.u32p, C.c_int] + [C.c_int] * 5 + [i32p, i32p]
    return L


@pytest.fixture(autouse=True)
def restore_switch_and_routing():
    """both are process-global: every test leaves the library's defaults behind"""
    assert gpu.extra_tile_cols() == X.T
    try:
        yield
    finally:
        gpu.set_extra_routing(*DEFAULT_ROUTING)
        gpu.set_extra_device(-1)


def walk(H, cig, q, t, sc):
    f, g = np.zeros(6, np.int32), np.zeros(6, np.int32)
    cg = np.ascontiguousarray(cig, np.uint32) if len(cig) else np.zeros(1, np.uint32)
    H.h_extra_walk_both(q.ctypes.data, t.ctypes.data, cg, len(cig), *[int(v) for v in sc], f, g)
    return g


def run_bytes(ctx, cases):
    """cases of one score through wm_extra_batch"""
    jobs = np.zeros(len(cases), gpu.EXTRA_JOB_DTYPE)
    seqs, cigs = [], [np.zeros(0, np.uint32)]
    at = ops = 0
    for i, (_, cig, q, t, _) in enumerate(cases):
        jobs[i] = (at, at + len(q), ops, len(cig))
        seqs += [q, t]; at += len(q) + len(t); cigs.append(cig); ops += len(cig)
    return ctx.extra_batch(cases[0][4], jobs, np.concatenate(seqs), np.concatenate(cigs).astype(np.uint32))


def by_score(cases):
    groups = {}
    for c in cases:
        groups.setdefault(tuple(c[4]), []).append(c)
    return list(groups.values())


@pytest.fixture(scope="module")
def EXPECTED(H):
    """computed once: every byte-form case with what wm_extra_walk gives"""
    cases = X.make_cases() + X.batch70()
    return [(c, walk(H, c[1], c[2], c[3], c[4])) for c in cases]


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_every_named_case_equals_wm_extra_walk(ctx, EXPECTED, long_min, tile):
    gpu.set_extra_routing(long_min, tile)
    assert gpu.extra_tile_cols() == tile
    want = {c[0]: w for c, w in EXPECTED}
    n = 0
    for group in by_score([c for c, _ in EXPECTED]):
        out = run_bytes(ctx, group)
        for c, got in zip(group, out):
            assert np.array_equal(got, want[c[0]]), (c[0], long_min, tile, got, want[c[0]])
            n += 1
    assert n == len(EXPECTED) > 130


@pytest.mark.skipif(not W.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("long_min,tile", [(ALL_SHORT, X.T), (ALL_LONG, 64)])
def test_final_cigars_equal_the_references_own_mm_update_extra(ctx, long_min, tile):
    gpu.set_extra_routing(long_min, tile)
    cases, wants = X.through_the_reference(W.ref(), X.raw_alignments_for_the_reference())
    assert len(cases) > 250
    for score in sorted(set(c[4] for c in cases)):
        G = [(c, w) for c, w in zip(cases, wants) if c[4] == score]
        out = run_bytes(ctx, [c for c, _ in G])
        for (c, w), got in zip(G, out):
            assert (int(got[2]), int(got[1]), int(got[3]), int(got[0])) == w, (c[0], score, got, w)      # blen, mlen, n_ambi, dp_max


def test_the_default_routing_sends_a_long_cigar_over_many_wavefronts_and_gives_the_same(ctx, H):
    """under the library's own thresholds: an asm20-like alignment of 40 000 columns (long class: 79 tiles + combine) beside short ones"""
    ops = []
    rng = np.random.default_rng(9)
    for k in range(20):
        ops += [(X.M, 2000), (int(rng.choice([X.I, X.D])), int(rng.integers(1, 300)))]
    long_case = ("long_40k",) + X.build(ops, seed=9, mm_rate=0.02, t_n=[5, 30000], q_n=[777]) + (X.ASM20,)
    short = [c for c in X.make_cases() if tuple(c[4]) == X.ASM20]
    out = run_bytes(ctx, short + [long_case])
    for c, got in zip(short + [long_case], out):
        want = walk(H, c[1], c[2], c[3], c[4])
        assert np.array_equal(got, want), (c[0], got, want)


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def POS(H):
    """the position cases: their contigs as a small uploaded index, their read resident behind a lead; expected = wm_extra_walk over the operands spelled out.
    A context of its own: a mapper replaces the resident reads of the context it maps on."""
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
        want.append(walk(H, cig, q, t, score))
    yield ctx, P, lead, want
    idx.close()
    ctx.close()


@pytest.mark.parametrize("long_min,tile", ROUTES)
def test_position_form_equals_wm_extra_walk(POS, long_min, tile):
    ctx, P, lead, want = POS
    gpu.set_extra_routing(long_min, tile)
    for score in sorted(set(tuple(p[6]) for p in P)):
        G = [(rid, p) for rid, p in enumerate(P) if tuple(p[6]) == score]
        jobs = np.zeros(len(G), gpu.EXTRA_POS_DTYPE)
        cigs, ops = [], 0
        for i, (rid, p) in enumerate(G):
            jobs[i] = (lead, len(p[2]), p[3], rid, p[5], ops, len(p[1]))
            cigs.append(p[1]); ops += len(p[1])
        out = ctx.extra_batch_pos(score, jobs, np.concatenate(cigs))
        for (rid, p), got in zip(G, out):
            assert np.array_equal(got, want[rid]), (p[0], long_min, tile, got, want[rid])


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_name_the_job(ctx, POS, H):
    ok = X.build([(X.M, 100)], seed=1)
    cig, q, t = ok
    seqs = np.concatenate([q, t])
    two = np.zeros(2, gpu.EXTRA_JOB_DTYPE)
    two[0] = (0, len(q), 0, 1); two[1] = (0, len(q), 0, 1)
    # the int32 limit, tripped with a large match on a 100-column job: 100 * match + 0 gaps > 2^30; the largest match below it is exact
    big = gpu.EXTRA_MAX_ABS // 100
    out = ctx.extra_batch((big, -4, -1, 4, 2), two, seqs, cig)
    assert np.array_equal(out[1], walk(H, cig, q, t, (big, -4, -1, 4, 2))) and out[1][0] == 100 * big
    for sc in ((big + 1, -4, -1, 4, 2), (2, -(big + 1), -1, 4, 2), (2, -4, big + 1, 4, 2)):
        with pytest.raises(gpu.WmError, match="job 0.*WM_EXTRA_MAX_ABS"):
            ctx.extra_batch(sc, two, seqs, cig)
    gapc = np.array([50 << 4, (1 << 27) << 4 | 2, 50 << 4], np.uint32)          # one D op whose q + e * len alone passes the limit
    with pytest.raises(gpu.WmError, match="job 0.*WM_EXTRA_MAX_ABS"):
        ctx.extra_batch((2, -4, -1, 4, 8), np.array([(0, len(q), 0, 3)], gpu.EXTRA_JOB_DTYPE), seqs, gapc)
    # a CIGAR that consumes more query / target than seqs holds behind the offsets
    bad = two.copy(); bad[1] = (len(seqs) - 99, len(q), 0, 1)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.extra_batch(X.ONT, bad, seqs, cig)
    bad = two.copy(); bad[1] = (0, len(seqs) - 99, 0, 1)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.extra_batch(X.ONT, bad, seqs, cig)
    # ops beyond n_ops
    bad = two.copy(); bad[1] = (0, len(q), 1, 1)
    with pytest.raises(gpu.WmError, match="job 1"):
        ctx.extra_batch(X.ONT, bad, seqs, cig)
    bad = two.copy(); bad[0] = (0, len(q), 0, -1)
    with pytest.raises(gpu.WmError, match="job 0"):
        ctx.extra_batch(X.ONT, bad, seqs, cig)
    # n_cigar == 0 is valid and gives zeros, whatever the offsets say
    z = np.array([(4000000000, 4000000000, 0, 0)], gpu.EXTRA_JOB_DTYPE)
    assert not ctx.extra_batch(X.ONT, z, seqs, cig).any()
    # position form: the target past its contig's end, a contig that does not exist, the (sub)read outside the resident reads, a query far outside two-strand space
    pctx, P, lead, _ = POS
    last = len(P) - 1
    clen, L = len(P[last][4]), len(P[0][2])
    m100 = np.array([100 << 4], np.uint32)
    good = (lead, L, 0, last, clen - 100, 0, 1)
    assert pctx.extra_batch_pos(X.ONT, np.array([good], gpu.EXTRA_POS_DTYPE), m100)[0][5] == 100
    for j in ((lead, L, 0, last, clen - 99, 0, 1), (lead, L, 0, len(P), 0, 0, 1), (lead, L, 0, last, -1, 0, 1), (lead + 12, L, 0, last, 0, 0, 1), (-1, L, 0, last, 0, 0, 1),
              (lead, L, 2 * L, last, 0, 0, 1), (lead, L, -100, last, 0, 0, 1)):
        with pytest.raises(gpu.WmError, match="job 1"):
            pctx.extra_batch_pos(X.ONT, np.array([good, j], gpu.EXTRA_POS_DTYPE), m100)


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["ont_short", "hifi", "asm20"])
def test_mapper_with_the_scans_on_the_device_gives_the_golden_and_the_same_text(ctx, name):
    tmp = tempfile.mkdtemp()
    preset, fa, kf, k, reads = E.make_golden.inputs(name, tmp)
    idx = gpu.Index(fa, kf, k=k, w=50, n_threads=8)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, preset, gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG)
    names = ["read%d" % i for i in range(len(reads))]
    try:
        gpu.set_extra_device(0)
        gpu.extra_stats(reset=True)
        text0, hits0, cigars0, first0 = m.map(names, reads)
        assert gpu.extra_stats()["deferred"] == 0
        gpu.set_extra_device(1)
        assert gpu.extra_device_enabled()
        text1, hits1, cigars1, first1 = m.map(names, reads)
        st = gpu.extra_stats()
    finally:
        m.close()
        idx.close()
    E.compare(name, hits1, cigars1, first1, reads)
    assert text1 == text0 and np.array_equal(hits1, hits0) and np.array_equal(cigars1, cigars0)
    # every read of a wm_map_reads call is resident (slot 0 always has its slab), so no region may fall back to the host walk
    assert st["deferred"] > 0 and st["on_device"] == st["deferred"] and st["on_host"] == 0 and st["calls"] > 0 and st["columns"] > 0


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
        gpu.set_extra_device(0)
        off = both_slots()
        gpu.set_extra_device(1)
        gpu.extra_stats(reset=True)
        on = both_slots()
        st = gpu.extra_stats()
    finally:
        m.close()
        idx.close()
    assert on == off and all(t.count(b"\n") >= len(reads) for t in on)
    assert st["on_device"] == st["deferred"] > 0 and st["on_host"] == 0 and st["calls"] >= 2

"""The splice-aware extension at its edges on the GPU: every case of tests/exts2cases.py through wm_ksw_exts2_batch against the oracle's ksw_exts2_sse
(pinned to the reference by tests/test_oracle_vs_ref.py, to the emulated kernel by tests/test_exts2_edges_emu.py); the batch geometries of its four
kernels; its argument checks; one job per alignment path whose maximum lies beyond target base 2^20; and the mapper's splitting of a splice-mode call into
groups that fit the arena."""
import ctypes as C
import os
import tempfile
import numpy as np
import pytest
import wmtest as W
import exts2cases as XC
from winnowmap_amd import gpu, synth

pytestmark = [pytest.mark.gpu]

CASES = XC.edge_cases()
_EXPECT = {}


def oracle_of(c):
    if c["name"] not in _EXPECT:
        _EXPECT[c["name"]] = W.o_ksw_exts2(c["q"], c["t"], mat=W.simple_mat(c["a"], c["b"], c["sc_ambi"]), q=c["q_"], e=c["e"], q2=c["q2"], noncan=c["noncan"],
                                           zdrop=c["zdrop"], junc_bonus=c["junc_bonus"], flag=c["flag"], junc=c["junc"])
    return _EXPECT[c["name"]]


@pytest.fixture(scope="module")
def ctx():
    c = gpu.Context(0, 1 << 30)
    yield c
    c.close()


def score_of(c):
    return gpu.KswScore(c["a"], -c["b"], c["sc_ambi"], c["q_"], c["e"], c["q2"], 0)


def pack(cs):
    jobs, seqs = gpu.pack_jobs([(c["q"], c["t"], dict(w=-1, zdrop=c["zdrop"], end_bonus=0, flag=c["flag"])) for c in cs])
    junc = None
    if any(c["junc"] is not None for c in cs):                 # (jobs with and without junction bits in one batch)
        junc = np.zeros(len(seqs), np.uint8)
        for j, c in zip(jobs, cs):
            if c["junc"] is not None:
                junc[j["t_off"]:j["t_off"] + j["tlen"]] = c["junc"]
    return jobs, seqs, junc


def check(cs, res, pool):
    bad = []
    for i, c in enumerate(cs):
        o, g = oracle_of(c), res[i]
        cig = pool[g["cig_off"]:g["cig_off"] + g["n_cigar"]]
        if any(int(g[k]) != o[k] for k in W.EZ_FIELDS) or not np.array_equal(cig, o["cigar"]):
            bad.append((i, c["name"], {k: (int(g[k]), o[k]) for k in W.EZ_FIELDS if int(g[k]) != o[k]}, W.cigar_str(cig)[:40], W.cigar_str(o["cigar"])[:40]))
    assert not bad, (len(bad), bad[:6])


def test_every_case_matches_oracle(ctx):
    groups = {}
    for c in CASES:
        groups.setdefault(XC.scoring_key(c), []).append(c)
    assert len(groups) >= 20
    for cs in groups.values():
        jobs, seqs, junc = pack(cs)
        res, pool = ctx.ksw_exts2_batch(score_of(cs[0]), cs[0]["noncan"], cs[0]["junc_bonus"], jobs, seqs, junc)
        check(cs, res, pool)


def _raw(ctx, sc, noncan, jb, jobs, seqs, cap):
    L = gpu.lib()
    L.wm_ksw_exts2_batch.argtypes = [C.c_void_p, C.POINTER(gpu.KswScore), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                     C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    jobs = np.ascontiguousarray(jobs, gpu.KSW_JOB_DTYPE)
    res = np.zeros(len(jobs), gpu.KSW_RES_DTYPE)
    pool = np.zeros(max(cap, 1), np.uint32)
    used = C.c_size_t(0)
    rc = L.wm_ksw_exts2_batch(ctx._h, C.byref(sc), noncan, jb, len(jobs), jobs.ctypes.data, seqs.ctypes.data, seqs.nbytes, None, res.ctypes.data, pool.ctypes.data, cap, C.byref(used))
    return rc, res, pool, used.value


def _tiny():
    """jobs of a few bases with the preset's scoring and no junction bits; the extensions with no positive cell (no CIGAR: an empty slot for the gather) go
    first, in the middle and last"""
    key = XC.scoring_key(XC._case("x", [0], [0]))
    tiny = [c for c in CASES if XC.scoring_key(c) == key and c["junc"] is None and len(c["q"]) + len(c["t"]) <= 60 and not c["name"].startswith("nopos")]
    nopos = [c for c in CASES if c["name"].startswith("nopos")]
    assert len(tiny) >= 40 and len(nopos) == 3
    return tiny, nopos


@pytest.mark.parametrize("n_jobs", [1, 63, 64, 65, 1024, 1025, 2049])
def test_batch_geometry(ctx, n_jobs):
    """one wavefront per job; the backtrack kernel runs 64 threads per block, the scan is one block of 1024 threads, the gather one block per job"""
    tiny, nopos = _tiny()
    cs = [tiny[i % len(tiny)] for i in range(n_jobs)]
    cs[0] = nopos[0]
    cs[n_jobs // 2] = nopos[1 if n_jobs > 2 else 0]
    cs[-1] = nopos[2 if n_jobs > 2 else 0]
    jobs, seqs, _ = pack(cs)
    res, pool = ctx.ksw_exts2_batch(score_of(cs[0]), 9, 9, jobs, seqs)
    check(cs, res, pool)
    assert int(res["n_cigar"].sum()) == len(pool) and res["n_cigar"][0] == 0 and res["n_cigar"][-1] == 0


def test_cigar_cap_and_a_shared_target(ctx):
    tiny, nopos = _tiny()
    cs = tiny[:20] + nopos[:1] + tiny[20:30]
    jobs, seqs, _ = pack(cs)
    sc = score_of(cs[0])
    total = sum(len(oracle_of(c)["cigar"]) for c in cs)
    rc, res, pool, used = _raw(ctx, sc, 9, 9, jobs, seqs, total)                    # a pool of exactly the size needed
    assert rc == 0 and used == total
    check(cs, res, pool)
    rc, _, _, used = _raw(ctx, sc, 9, 9, jobs, seqs, total - 1)                     # one op less: WM_ENOMEM, and the need comes back
    assert rc == -3 and used == total and b"cigar_pool too small" in gpu.lib().wm_last_error()
    # two jobs on one target
    a, b = tiny[3], tiny[4]
    seqs2 = np.concatenate([a["q"], b["q"], a["t"]])
    c2 = dict(b, name=b["name"] + "_on_" + a["name"], t=a["t"])
    jobs2 = np.zeros(2, gpu.KSW_JOB_DTYPE)
    t_off = len(a["q"]) + len(b["q"])
    jobs2[0] = (0, t_off, len(a["q"]), len(a["t"]), -1, a["zdrop"], 0, a["flag"])
    jobs2[1] = (len(a["q"]), t_off, len(b["q"]), len(a["t"]), -1, b["zdrop"], 0, b["flag"])
    res, pool = ctx.ksw_exts2_batch(sc, 9, 9, jobs2, seqs2)
    check([a, c2], res, pool)


def test_argument_checks(ctx):
    """the scoring sets the reference answers with a reset result (src/ksw2_exts2_sse.c:66, :84) — the N score below -2 (q + e) among them — and a target
    longer than WM_KSW_MAX_TLEN are refused with WM_EINVAL by every alignment entry point that takes them"""
    c0 = CASES[0]
    jobs, seqs, _ = pack([c0])
    for nm, (a, b, q, e, q2, amb) in XC.REJECTED:
        with pytest.raises(gpu.WmError):
            ctx.ksw_exts2_batch(gpu.KswScore(a, -b, amb, q, e, q2, 0), 9, 9, jobs, seqs)
        assert {"b": b"mismatch penalty above", "a": b"N score below", "q": b"q2 > q + e"}[nm[0]] in gpu.lib().wm_last_error(), nm
    ctx.ksw_exts2_batch(gpu.KswScore(1, -2, -6, 2, 1, 32, 0), 9, 9, jobs, seqs)                   # on the limit: taken
    too_long = (1 << 28) + 1
    j = jobs.copy()
    j["tlen"] = too_long
    rc, _, _, _ = _raw(ctx, score_of(c0), 9, 9, j, seqs, 16)
    assert rc == -2 and b"WM_KSW_MAX_TLEN = 268435456" in gpu.lib().wm_last_error()
    # wm_ksw_batch / wm_ksw_dev_prepare / wm_ksw_extd2 (the operands must exist there: zero pages nobody reads, the check comes first)
    big = np.zeros(too_long + 8, np.uint8)
    jb = np.zeros(1, gpu.KSW_JOB_DTYPE)
    jb[0] = (0, 8, 8, too_long, 10, 400, -1, 0x40)
    L = gpu.lib()
    sc = gpu.KswScore(2, -4, -1, 4, 2, 24, 1)
    res = np.zeros(1, gpu.KSW_RES_DTYPE)
    pool = np.zeros(16, np.uint32)
    used = C.c_size_t(0)
    L.wm_ksw_batch.argtypes = [C.c_void_p, C.POINTER(gpu.KswScore), C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]
    assert L.wm_ksw_batch(ctx._h, C.byref(sc), 1, jb.ctypes.data, big.ctypes.data, big.nbytes, res.ctypes.data, pool.ctypes.data, 16, C.byref(used)) == -2
    assert b"WM_KSW_MAX_TLEN" in L.wm_last_error()
    with pytest.raises(gpu.WmError):
        ctx.ksw_prepare(sc, jb, big)
    assert b"WM_KSW_MAX_TLEN" in L.wm_last_error()


def test_exts2_maximum_beyond_2_to_20_target_bases(ctx):
    """a 1 048 600-base intron between a 20- and a 60-base exon (the maximum stands at target base 1 048 679; 100 MB of traceback), and the same job with
    1 048 400 bases, below 2^20. One wavefront walks 1 048 769 rows per job: 8.5 s for the two on an MI355X, more than the rest of this file together (4 s) —
    the defect this pins does not exist below 2^20 target bases"""
    for n in (1048400, 1048600):
        c = XC.long_intron_case(n)
        o = oracle_of(c)
        assert (o["max"], o["max_q"], o["max_t"]) == (48, 79, n + 79) and W.cigar_str(o["cigar"]) == "20M%dN60M" % n
        jobs, seqs, _ = pack([c])
        res, pool = ctx.ksw_exts2_batch(score_of(c), c["noncan"], c["junc_bonus"], jobs, seqs)
        check([c], res, pool)


def test_extd2_maximum_beyond_2_to_20_target_bases():
    """query == target of 1 048 700 bases under a band of 10, extension with exact maximum: the 4-pair packed class (ksw_packed_kernel.h), 67 MB of
    traceback; and the same at 1 048 500 bases. One wavefront walks 2 097 399 rows per job: 6.8 s for the two on an MI355X, also more than the rest of this file"""
    ctx = gpu.Context(0, 1 << 30)
    try:
        for n in (1048500, 1048700):
            c = XC.long_identity_case(n)
            o = W.o_ksw_extd2(c["q"], c["t"], mat=W.simple_mat(c["a"], c["b"], 1), q=c["q_"], e=c["e"], q2=c["q2"], e2=c["e2"], w=c["w"], zdrop=c["zdrop"],
                              end_bonus=c["end_bonus"], flag=c["flag"])
            assert (o["max"], o["max_q"], o["max_t"]) == (2 * n, n - 1, n - 1)
            jobs, seqs = gpu.pack_jobs([(c["q"], c["t"], dict(w=c["w"], zdrop=c["zdrop"], end_bonus=c["end_bonus"], flag=c["flag"]))])
            res, pool = ctx.ksw_batch(gpu.KswScore(c["a"], -c["b"], -1, c["q_"], c["e"], c["q2"], c["e2"]), jobs, seqs)
            g = res[0]
            assert all(int(g[k]) == o[k] for k in W.EZ_FIELDS), (n, {k: (int(g[k]), o[k]) for k in W.EZ_FIELDS if int(g[k]) != o[k]})
            assert np.array_equal(pool[g["cig_off"]:g["cig_off"] + g["n_cigar"]], o["cigar"])
        ran = {k: v[2] for k, v in ctx.kernel_stats().items() if v[2]}
        assert ran == {6: 2}, ran                                  # WM_KSW_P4 + EXACT * 4 + CLIP * 2: both jobs, and nothing else
    finally:
        ctx.close()


SPLIT_ARENA = 32 << 20


def test_mapper_splits_a_splice_call_into_groups_that_fit_the_arena():
    """GpuOpsCtx::exts2_batch cuts the requests of a call into groups whose unbanded traceback fits 0.6 of the context's arena: spliced reads mapped with an
    arena of SPLIT_ARENA bytes and with the default give the same hits and CIGARs, and the small run did split (wm_exts2_stats: more groups than calls)"""
    tmp = tempfile.mkdtemp()
    ref = synth.make_reference(1, 200000, 61, repeat_frac=0.0)
    reads = synth.make_transcripts(ref, 24, 62)
    fa = os.path.join(tmp, "ref.fa")
    synth.write_fasta(fa, ref, prefix="chr")
    names = [b"r%d" % i for i in range(len(reads))]
    seqs = [synth.codes_to_ascii(r) for r in reads]
    out = []
    for arena in (SPLIT_ARENA, 0):
        ctx = gpu.Context(0, arena)
        idx = gpu.Index(fa, None, k=15, w=25, n_threads=4)
        idx.upload(ctx)
        m = gpu.Mapper(ctx, idx, "splice", gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG)
        m.set_threads(1, arena)                                  # one context: the one created above
        gpu.exts2_stats(reset=True)
        text, hits, cigs, first = m.map(names, seqs)
        out.append((text, hits.copy(), cigs.copy(), first.copy(), gpu.exts2_stats()))
        m.close(); idx.close(); ctx.close()
    small, dflt = out
    assert small[0] == dflt[0] and np.array_equal(small[1], dflt[1]) and np.array_equal(small[2], dflt[2]) and np.array_equal(small[3], dflt[3])
    assert len(dflt[1]) >= 20 and int(np.sum((dflt[2] & 0xf) == 3)) >= 20
    assert dflt[4]["calls"] >= 1 and dflt[4]["groups"] == dflt[4]["calls"], dflt[4]
    assert small[4]["groups"] >= small[4]["calls"] + 1 and small[4]["groups"] >= 2, small[4]

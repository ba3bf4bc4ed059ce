"""GPU: self and all-vs-all mapping — -X, -D, --dual=no (MM_F_NO_DIAG / MM_F_NO_DUAL, skip_seed src/map.c:132-154) — end to end against the reference
binary with the same arguments, through gpu.Mapper (names handed to Mapper.map) and through the reference's CLI bound to the library (the file
loop), and the keyed batched operations against a restatement of collect_seed_hits. Every expectation comes from the reference or is restated here.

Each end-to-end test first checks the EXPECTED output itself, so that a pass means something: the reference's plain run holds a full-length self hit
for every read; its -X output holds none of those, no record whose query name is strcmp-greater than its target name, and at least one record that
pairs a read with itself off the diagonal (the MM_SEED_SELF path, src/align.c:677)."""
import ctypes as C
import os
import subprocess
import tempfile
import time

import numpy as np
import pytest

import wmtest as W
from winnowmap_amd import gpu, parity, synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_ref")
WM_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_wm")
need_ref = pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/winnowmap_ref not built")
need_wm = pytest.mark.skipif(not os.path.exists(WM_BIN), reason="oracle/_ref/winnowmap_wm not built")
BASE = gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG
THREADS = 16


def _run(binary, args, env=None):
    e = dict(os.environ)
    e.update(env or {})
    t0 = time.time()
    p = subprocess.run([binary] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=1200)
    assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
    return p.stdout, time.time() - t0


def _name(i):
    """names of mixed shapes: their strcmp order is neither the file's nor the numbers'"""
    return (b"r%d" % i, b"read_%04d" % i, b"r%d/ccs" % i, b"R%d" % i)[i % 4]


def _write(path, names, seqs):
    with open(path, "wb") as f:
        for n, s in zip(names, seqs):
            f.write(b">" + n + b"\n" + s + b"\n")


def _paf(text):
    return [ln.split(b"\t") for ln in text.split(b"\n") if ln and not ln.startswith(b"@")]


def _full_self(f):
    """a PAF record that maps a read onto the whole of itself"""
    return f[0] == f[5] and f[4] == b"+" and int(f[2]) == 0 and int(f[3]) == int(f[1]) and int(f[7]) == 0 and int(f[8]) == int(f[6])


def _check_expected(plain, ava, names, need_off_diag=True):
    """the reference's own outputs have the properties that make the comparison worth something (see the module docstring)"""
    with_self = {f[0] for f in _paf(plain) if _full_self(f)}
    assert with_self == set(names), (len(with_self), len(names))
    recs = _paf(ava)
    assert not any(_full_self(f) for f in recs)
    assert not any(f[0] > f[5] for f in recs)                  # (bytes compare as unsigned chars, like strcmp; the names hold no NUL)
    off_diag = sum(1 for f in recs if f[0] == f[5])
    assert off_diag >= 1 or not need_off_diag, "no off-diagonal self pair: the MM_SEED_SELF path is not exercised"
    return len(recs), off_diag


@pytest.fixture(scope="module")
def ava():
    """1 000 synthetic ONT reads at ~7x over a 1.2 Mb genome: 500 of 12 kb (the windowed MCAS path) + 500 of 4 kb (the one-stage path); reads file = reference file"""
    tmp = tempfile.mkdtemp()
    ref = synth.make_reference(2, 600000, 51, repeat_frac=0.08)
    reads = synth.make_reads(ref, 500, 12000, 52, profile="ont")[0] + synth.make_reads(ref, 500, 4000, 53, profile="ont")[0]
    order = np.random.default_rng(54).permutation(len(reads))   # long and short reads interleaved in the file
    seqs = [synth.codes_to_ascii(reads[i]) for i in order]
    names = [_name(i) for i in range(len(seqs))]
    fa = os.path.join(tmp, "reads.fa")
    _write(fa, names, seqs)
    fa300 = os.path.join(tmp, "reads300.fa")
    _write(fa300, names[:300], seqs[:300])
    plain, _ = _run(REF_BIN, ["-t", str(THREADS), "-cx", "map-ont", fa, fa])
    ctx = gpu.Context(0, 24 << 30)
    idx = gpu.Index(fa, None, k=15, w=50, n_threads=THREADS)
    idx.upload(ctx)
    yield dict(tmp=tmp, fa=fa, fa300=fa300, names=names, seqs=seqs, plain=plain, ctx=ctx, idx=idx)
    idx.close()
    ctx.close()


def _mapper_text(ctx, idx, preset, flag, names, seqs):
    m = gpu.Mapper(ctx, idx, preset, flag)
    m.set_threads(THREADS, 24 << 30)
    t0 = time.time()
    text, hits, _, _ = m.map(names, seqs)
    dt = time.time() - t0
    defined = parity.defined_names(names, m.rep_len_defined())
    m.close()
    return text, defined, dt


@need_ref
@need_wm
@pytest.mark.parametrize("switch,bits", [("-X", gpu.MM_F_AVA), ("-D", gpu.MM_F_NO_DIAG), ("--dual=no", gpu.MM_F_NO_DUAL)])
def test_all_vs_all_1000_reads_paf(ava, switch, bits):
    A = ava
    args = ["-t", str(THREADS), switch, "-cx", "map-ont", A["fa"], A["fa"]]
    want, t_ref = _run(REF_BIN, args)
    assert want != A["plain"]
    if switch == "-X":
        n_rec, off_diag = _check_expected(A["plain"], want, A["names"])
        print("reference -X: %d records, %d off-diagonal self pairs, %.1f s at -t %d" % (n_rec, off_diag, t_ref, THREADS))
    elif switch == "-D":
        # the reference compares a contig's length with the length of the sequence it SEEDS (qlen_sum, src/map.c:346-364): a window's inside stage 1.
        # So -D changes the reads below the 10-kb MCAS gate and no others; restated, not "fixed"
        short = {n for n, s in zip(A["names"], A["seqs"]) if len(s) < 10000}
        gp, gw = parity.group_by_read(A["plain"]), parity.group_by_read(want)
        changed = {n for n in A["names"] if gp.get(n) != gw.get(n)}
        assert changed == short, (len(changed), len(short))
    text, defined, dt = _mapper_text(A["ctx"], A["idx"], "map-ont", BASE | bits, A["names"], A["seqs"])
    d = parity.diff_texts(want, text, defined=defined)
    bases = sum(len(s) for s in A["seqs"])
    print("%s through gpu.Mapper: %d reads, %d records, %.2f s = %.0f reads/s, %.5f Gbp/s (reference: %.1f s at -t %d)" %
          (switch, len(A["seqs"]), d["hits"], dt, len(A["seqs"]) / dt, bases / dt / 1e9, t_ref, THREADS))
    assert d["reads"] >= 800 and d["mismatches"] == 0, d
    got, _ = _run(WM_BIN, args)
    d = parity.diff_texts(want, got)
    assert d["reads"] >= 800 and d["mismatches"] == 0, d


@need_ref
@need_wm
def test_all_vs_all_300_reads_sam(ava):
    A = ava
    args = ["-t", str(THREADS), "-X", "-ax", "map-ont", A["fa300"], A["fa300"]]
    want, _ = _run(REF_BIN, args)
    got, _ = _run(WM_BIN, args)
    d = parity.diff_texts(want, got, sam=True)
    assert d["reads"] == 300 and d["hits"] >= 300 and d["mismatches"] == 0, d
    ctx = A["ctx"]
    idx = gpu.Index(A["fa300"], None, k=15, w=50, n_threads=THREADS)
    idx.upload(ctx)
    try:
        text, defined, _ = _mapper_text(ctx, idx, "map-ont", gpu.MM_F_CIGAR | gpu.MM_F_OUT_SAM | gpu.MM_F_AVA, A["names"][:300], A["seqs"][:300])
    finally:
        A["idx"].upload(ctx)          # the module's index back on the context
        idx.close()
    d = parity.diff_texts(want, text, sam=True, defined=defined)
    assert d["reads"] == 300 and d["mismatches"] == 0, d


@need_ref
def test_assembly_self_alignment_DP_asm20_device_built_index():
    """4 contigs of 500 kb with segmental repeats against themselves, -DP -cx asm20, the index built on the device"""
    tmp = tempfile.mkdtemp()
    rng = np.random.default_rng(61)
    ctg = synth.make_reference(4, 500000, 62)
    for (a, pa, b, pb, ln) in ((0, 50000, 2, 300000, 30000), (1, 100000, 1, 350000, 20000), (3, 10000, 0, 420000, 25000)):     # segmental duplications, within and between contigs
        ctg[b][pb:pb + ln] = synth.mutate_codes(ctg[a][pa:pa + ln].copy(), rng, 0.03, 0.0, 0.0)[:ln]
    ctg[2][100000:115000] = synth.revcomp_codes(synth.mutate_codes(ctg[3][200000:215000].copy(), rng, 0.02, 0.0, 0.0))[:15000]
    names = [b"ctg_%d" % i for i in (3, 10, 2, 1)]                               # file order is not name order
    seqs = [synth.codes_to_ascii(c) for c in ctg]
    fa = os.path.join(tmp, "asm.fa")
    _write(fa, names, seqs)
    args = ["-t", str(THREADS), "-DP", "-cx", "asm20", fa, fa]
    want, _ = _run(REF_BIN, args)
    recs = _paf(want)
    assert len(recs) >= 6 and any(f[0] != f[5] for f in recs)                    # the duplications between contigs ...
    assert any(f[0] == f[5] and not _full_self(f) for f in recs)                 # ... and self pairs off the diagonal (the duplication inside ctg_10)
    _, k, w = gpu.mapopt_preset("asm20")
    ctx = gpu.Context(0, 16 << 30)
    idx, _ = gpu.Index.build_on_device(ctx, fa, None, k=k, w=w, n_threads=THREADS)
    idx.upload(ctx)
    text, defined, _ = _mapper_text(ctx, idx, "asm20", BASE | gpu.MM_F_NO_DIAG | gpu.MM_F_ALL_CHAINS, names, seqs)
    idx.close(); ctx.close()
    d = parity.diff_texts(want, text, defined=defined)
    assert d["reads"] == 4 and d["mismatches"] == 0, d
    if os.path.exists(WM_BIN):
        got, _ = _run(WM_BIN, args)
        d = parity.diff_texts(want, got)
        assert d["reads"] == 4 and d["mismatches"] == 0, d


@need_ref
@pytest.mark.parametrize("same_len", [True, False])
def test_reads_against_a_reference_with_a_contig_named_like_a_read(same_len):
    """skip_seed needs the name AND the length to agree (src/map.c:141): one contig carries a read's name — once with that read's length, once not"""
    tmp = tempfile.mkdtemp()
    ref = synth.make_reference(2, 300000, 71, repeat_frac=0.08)
    reads = synth.make_reads(ref, 20, 12000, 72, profile="ont")[0] + synth.make_reads(ref, 20, 4000, 73, profile="ont")[0]
    seqs = [synth.codes_to_ascii(r) for r in reads]
    names = [_name(i) for i in range(len(seqs))]
    twins = (3, 25)                                                             # a long and a short read are also contigs of the reference
    cn = [b"chrA", b"chrB"] + [names[i] for i in twins]
    cs = [synth.codes_to_ascii(c) for c in ref] + [seqs[i] if same_len else seqs[i] + b"ACGTTGCA" for i in twins]
    fa, rq = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fa")
    _write(fa, cn, cs)
    _write(rq, names, seqs)
    ctx = gpu.Context(0, 8 << 30)
    idx = gpu.Index(fa, None, k=15, w=50, n_threads=THREADS)
    idx.upload(ctx)
    plain, _ = _run(REF_BIN, ["-t", "4", "-cx", "map-ont", fa, rq])
    n_differs = 0
    for switch, bits in (("-D", gpu.MM_F_NO_DIAG), ("-X", gpu.MM_F_AVA)):
        args = ["-t", "4", switch, "-cx", "map-ont", fa, rq]
        want, _ = _run(REF_BIN, args)
        n_differs += want != plain
        if switch == "-D":
            # the short twin (one-stage path: qlen = the read's length) loses its diagonal hit exactly when the lengths agree
            short = names[twins[1]]
            has_diag = any(f[0] == short and f[5] == short and int(f[2]) == 0 and int(f[3]) == int(f[1]) for f in _paf(want))
            assert has_diag == (not same_len)
        text, defined, _ = _mapper_text(ctx, idx, "map-ont", BASE | bits, names, seqs)
        # (-X keeps only the targets whose name is not smaller than the read's: the reference prints records for 10 / 11 of the 40 reads here)
        n_min = 38 if switch == "-D" else 8
        d = parity.diff_texts(want, text, defined=defined)
        assert d["reads"] >= n_min and d["mismatches"] == 0, (switch, d)
        if os.path.exists(WM_BIN):
            got, _ = _run(WM_BIN, args)
            d = parity.diff_texts(want, got)
            assert d["reads"] >= n_min and d["mismatches"] == 0, (switch, d)
    assert n_differs >= 1
    idx.close(); ctx.close()


@need_ref
def test_split_prefix_with_X_over_two_parts():
    """every part of a split index ranks its own contig names: the key of a read is made per part"""
    tmp = tempfile.mkdtemp()
    ref = synth.make_reference(1, 200000, 91, repeat_frac=0.05)
    reads = synth.make_reads(ref, 30, 12000, 92, profile="ont")[0] + synth.make_reads(ref, 30, 4000, 93, profile="ont")[0]
    order = np.random.default_rng(94).permutation(len(reads))
    seqs = [synth.codes_to_ascii(reads[i]) for i in order]
    names = [_name(i) for i in range(len(seqs))]
    fa = os.path.join(tmp, "reads.fa")
    _write(fa, names, seqs)
    args = ["-t", "1", "-I", "250k", "--split-prefix", os.path.join(tmp, "sp"), "-X", "-cx", "map-ont", fa, fa]
    want, _ = _run(REF_BIN, args)
    one, _ = _run(REF_BIN, ["-t", "4", "-cx", "map-ont", fa, fa])
    _check_expected(one, want, names, need_off_diag=False)     # (60 reads at 2.4x: no read overlaps itself here; the 1 000-read test asks for that)
    ctx = gpu.Context(0, 8 << 30)
    parts = gpu.build_index_parts(fa, None, 15, 50, 250000)
    assert len(parts) == 2
    opt, _, _ = gpu.mapopt_preset("map-ont")
    opt.flag |= BASE | gpu.MM_F_AVA
    outp = os.path.join(tmp, "ours.paf")
    st = gpu.map_file_split(ctx, parts, opt, 8, fa, outp)                       # (the reference prints records for 42 of the 60 reads)
    assert st["reads"] == len(seqs)
    d = parity.diff_texts(want, open(outp, "rb").read())
    assert d["reads"] >= 40 and d["mismatches"] == 0, d
    for p in parts:
        p.close()
    ctx.close()
    if os.path.exists(WM_BIN):
        args[5] = os.path.join(tmp, "sp2")
        got, _ = _run(WM_BIN, args)
        d = parity.diff_texts(want, got)
        assert d["reads"] >= 40 and d["mismatches"] == 0, d


# ---- the keyed batched operations ----------------------------------------------------------------------------------------------------------
M128 = np.dtype([("x", np.uint64), ("y", np.uint64)])
NO_DIAG, NO_DUAL = gpu.MM_F_NO_DIAG, gpu.MM_F_NO_DUAL
SEED_SELF = 1 << 43


def _restated_seed_hits(L, idx, cnames, clens, mx, my, qlen, max_occ, flag, qname):
    """collect_matches + collect_seed_hits before the sort (src/map.c:97-130, 222-251) with skip_seed (:132-154) on Python's bytes, which compare as
    strcmp does (unsigned chars, no NUL inside a name)"""
    ex, ey = [], []
    rep_st = rep_en = rep = 0
    t = C.c_int()
    for j in range(len(mx)):
        x, y = int(mx[j]), int(my[j])
        p = L.wm_index_get(idx._h, x >> 8, C.byref(t))
        q_pos, span = y & 0xffffffff, x & 0xff
        if t.value >= max_occ:
            en = (q_pos >> 1) + 1; st = en - span
            if st > rep_en:
                rep += rep_en - rep_st; rep_st, rep_en = st, en
            else:
                rep_en = en
            continue
        tand = (j > 0 and int(mx[j - 1]) >> 8 == x >> 8) or (j < len(mx) - 1 and int(mx[j + 1]) >> 8 == x >> 8)
        for h in range(t.value):
            r = int(p[h]); is_self = 0
            if qname is not None and flag & (NO_DIAG | NO_DUAL):
                rid = r >> 32
                same, greater = qname == cnames[rid], qname > cnames[rid]
                if (flag & NO_DIAG) and same and clens[rid] == qlen:
                    if (r & 0xffffffff) >> 1 == q_pos >> 1:
                        continue
                    if (r & 1) == (q_pos & 1):
                        is_self = 1
                if (flag & NO_DUAL) and greater:
                    continue
            rpos = (r & 0xffffffff) >> 1
            if (r & 1) == (q_pos & 1):
                X = (r & 0xffffffff00000000) | rpos; Y = span << 32 | q_pos >> 1
            else:
                X = 1 << 63 | (r & 0xffffffff00000000) | rpos; Y = span << 32 | (qlen - ((q_pos >> 1) + 1 - span) - 1)
            if tand:
                Y |= 1 << 42
            if is_self:
                Y |= SEED_SELF
            ex.append(X); ey.append(Y)
    rep += rep_en - rep_st
    return np.array(ex, np.uint64), np.array(ey, np.uint64), rep


def test_keyed_seed_and_window_batches_against_the_restatement():
    """10^3 jobs on one real index (250 reads indexed as contigs; jobs = whole reads, windows of reads, reads that are no contig): wm_seed_batch_keyed
    and wm_window_batch_keyed against the restatement + the oracle's sort and mm_chain_dp; unkeyed calls ignore the two bits"""
    tmp = tempfile.mkdtemp()
    ref = synth.make_reference(1, 150000, 101, repeat_frac=0.05)
    reads = synth.make_reads(ref, 150, 5000, 102, profile="ont")[0] + synth.make_reads(ref, 130, 2500, 103, profile="ont")[0]
    names = [_name(i) for i in range(len(reads))]
    n_ctg = 250                                                                 # the last 30 reads are not contigs: their names are absent from the index
    fa = os.path.join(tmp, "reads.fa")
    _write(fa, names[:n_ctg], [synth.codes_to_ascii(r) for r in reads[:n_ctg]])
    ctx = gpu.Context(0, 8 << 30)
    idx = gpu.Index(fa, None, k=15, w=50, n_threads=8)
    idx.upload(ctx)
    L = gpu.lib()
    L.wm_index_get.restype = C.POINTER(C.c_uint64)
    L.wm_index_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]
    cnames = [n.encode() for n in idx.names()]
    clens = [int(L.wm_index_seq_len(idx._h, i)) for i in range(n_ctg)]
    assert cnames == names[:n_ctg]
    rng = np.random.default_rng(104)
    jobs = []                                                                   # (read, start, len)
    for i in range(len(reads)):
        jobs.append((i, 0, len(reads[i])))                                      # the whole read: name and length agree with its contig
    while len(jobs) < 1000:
        i = int(rng.integers(0, len(reads))); ln = int(rng.integers(800, 2000)); st = int(rng.integers(0, len(reads[i]) - ln))
        jobs.append((i, st, ln))                                                # a window: the name agrees, the length does not
    qn = [names[i] for i, _, _ in jobs]
    keys = idx.query_keys(qn)
    assert all(int(keys[j][1]) == (jobs[j][0] < n_ctg) for j in range(len(jobs)))
    seqs = [np.ascontiguousarray(reads[i][st:st + ln]) for i, st, ln in jobs]
    minis = [W.o_sketch(bytes(s), 50, 15, rid=0) for s in seqs]
    nm = np.array([len(m[0]) for m in minis], np.int32)
    moff = np.concatenate([[0], np.cumsum(nm)[:-1]]).astype(np.uint64)
    allm = np.zeros((int(nm.sum()), 2), np.uint64)
    allm[:, 0] = np.concatenate([m[0] for m in minis]); allm[:, 1] = np.concatenate([m[1] for m in minis])
    qlen = np.array([ln for _, _, ln in jobs], np.int32)
    max_occ = 200
    par = dict(max_dist_x=5000, min_dist_x=1000, max_dist_y=5000, bw=500, max_skip=25, max_iter=5000, min_cnt=3, min_sc=40)
    J = np.zeros(len(jobs), gpu.WINDOW_JOB)
    J["seq_off"] = -1; J["len"] = qlen; J["stage_off"] = np.concatenate([[0], np.cumsum(qlen)[:-1]]); J["gap_scale"] = 1.0
    for k_, v in par.items():
        J[k_] = v
    stage = np.concatenate(seqs)
    n_self_total = 0
    for flag in (NO_DIAG, NO_DUAL, NO_DIAG | NO_DUAL):
        exp = [_restated_seed_hits(L, idx, cnames, clens, minis[j][0], minis[j][1], int(qlen[j]), max_occ, flag, qn[j]) for j in range(len(jobs))]
        cap = sum(len(e[0]) for e in exp) * 2 + 4096
        out, ooff, na, rl = ctx.seed_batch_keyed(allm, moff, nm, qlen, keys, max_occ, flag, cap)
        res, up, ap = ctx.window_batch_keyed(J, keys, stage, np.zeros((1, 2), np.uint64), max_occ, flag, cap, cap)
        for j, (ex, ey, rep) in enumerate(exp):
            sx, sy = W.o_radix_sort_128x(ex, ey)
            g = out[int(ooff[j]):int(ooff[j]) + int(na[j])]
            assert na[j] == len(ex) and rl[j] == rep, (flag, j, na[j], len(ex))
            assert np.array_equal(g[:, 0], sx) and np.array_equal(g[:, 1], sy), (flag, j)
            n_self_total += int(np.count_nonzero(sy & np.uint64(SEED_SELF)))
            eu, evx, evy = W.o_chain_dp(sx, sy, **par)
            r = res[j]
            assert r["n_anchors"] == len(ex) and r["rep_len"] == rep and r["n_u"] == len(eu) and r["n_v"] == len(evx), (flag, j, r)
            assert np.array_equal(up[r["u_off"]:r["u_off"] + r["n_u"]], eu), (flag, j)
            a = ap[r["a_off"]:r["a_off"] + r["n_v"]]
            assert np.array_equal(a[:, 0], evx) and np.array_equal(a[:, 1], evy), (flag, j)
    assert n_self_total > 0
    # without keys the two bits are ignored, as skip_seed ignores them for qname == NULL (src/map.c:135)
    cap = int(nm.sum()) * 64 + 4096
    base = ctx.seed_batch_keyed(allm, moff, nm, qlen, None, max_occ, 0, cap)
    bits = ctx.seed_batch_keyed(allm, moff, nm, qlen, None, max_occ, NO_DIAG | NO_DUAL, cap)
    assert all(np.array_equal(a, b) for a, b in zip(base, bits))
    wb = ctx.window_batch_keyed(J, None, stage, np.zeros((1, 2), np.uint64), max_occ, 0, cap, cap)
    wk = ctx.window_batch_keyed(J, None, stage, np.zeros((1, 2), np.uint64), max_occ, NO_DIAG | NO_DUAL, cap, cap)
    for j in range(len(jobs)):                  # (a job's slots in the result pools are taken with atomics: the offsets differ from call to call, the contents do not)
        rb, rk = wb[0][j], wk[0][j]
        assert all(rb[f] == rk[f] for f in ("n_anchors", "rep_len", "n_mini", "n_u", "n_v")), j
        assert np.array_equal(wb[1][rb["u_off"]:rb["u_off"] + rb["n_u"]], wk[1][rk["u_off"]:rk["u_off"] + rk["n_u"]]), j
        assert np.array_equal(wb[2][rb["a_off"]:rb["a_off"] + rb["n_v"]], wk[2][rk["a_off"]:rk["a_off"] + rk["n_v"]]), j
    # ... and the keyed -X answer is another one
    assert not np.array_equal(base[2], ctx.seed_batch_keyed(allm, moff, nm, qlen, keys, max_occ, NO_DIAG | NO_DUAL, cap)[2])
    idx.close(); ctx.close()

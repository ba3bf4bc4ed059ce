"""GPU: --heap-sort=yes (MM_F_HEAP_SORT), the heap-merged seed order of collect_seed_hits_heap (src/map.c:156-220), stage by stage and end to end.

The reads carry a tandem duplication inside the read (synth.make_dup_reads): two minimizers of one key and strand hit the same reference position, their
anchors share x, and the heap orders them differently from collect_seed_hits + radix_sort_128x — which is what a library that ignores the bit computes.
Every expectation comes from the reference: its heap driving the loop of src/map.c:169-218 restated in test_heapseed_emu.py, its binary, or a fixture written
from it (tests/golden/make_golden_heap.py)."""
import ctypes as C
import importlib.util
import os
import tempfile

import numpy as np
import pytest

import wmtest as W
import e2e_common as E
from winnowmap_amd import gpu, parity, synth
from test_selfmap_gpu import _run, _write, REF_BIN, WM_BIN, need_ref, need_wm, BASE
from test_selfmap_emu import _collect_seed_hits
from test_heapseed_emu import ref_heap_list, refheap, has_tie, _Tab  # noqa: F401  (refheap: a fixture)

pytestmark = pytest.mark.gpu
HEAP = gpu.MM_F_HEAP_SORT
FOR_ONLY = 0x100000
PAR = dict(max_dist_x=5000, min_dist_x=1000, max_dist_y=5000, bw=500, max_skip=25, max_iter=5000, min_cnt=3, min_sc=40)


def _names(n, prefix=b"d"):
    return [prefix + b"%d" % i for i in range(n)]


@pytest.fixture(scope="module")
def dup():
    """one random 200-kb contig; 200 duplicated reads below the 10 000-base MCAS gate (MAPQ and rl:i compared for every record) + 20 of ~15 kb (stage-1 windows,
    the stage-2 union sort)"""
    tmp = tempfile.mkdtemp()
    ref = synth.make_reference(1, 200000, 201)
    short = synth.make_dup_reads(ref, 200, 202)
    long_ = synth.make_dup_reads(ref, 20, 203, host=(13000, 14500))
    assert max(len(r) for r in short) < 10000 and min(len(r) for r in long_) >= 10000
    fa, rq, rs = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fa"), os.path.join(tmp, "short.fa")
    _write(fa, [b"chr0"], [synth.codes_to_ascii(c) for c in ref])
    seqs = [synth.codes_to_ascii(r) for r in short + long_]
    names = _names(len(seqs))
    _write(rq, names, seqs)
    _write(rs, names[:200], seqs[:200])
    ctx = gpu.Context(0, 8 << 30)
    idx = gpu.Index(fa, None, k=15, w=50, n_threads=8)
    idx.upload(ctx)
    yield dict(tmp=tmp, fa=fa, rq=rq, rs=rs, names=names, seqs=seqs, codes=short + long_, ctx=ctx, idx=idx)
    idx.close()
    ctx.close()


# ---- 5. stage by stage -----------------------------------------------------------------------------------------------------------------------
def _job_case(L, idx, mx, my, qlen, max_occ):
    """a job's minimizers and the lists of their keys as test_heapseed_emu's case dict (P: the lists one after the other)"""
    t = C.c_int()
    P, table = [], _Tab()
    for x in mx:
        k = int(x) >> 8
        if k in table:
            continue
        p = L.wm_index_get(idx._h, k, C.byref(t))
        table[k] = (len(P), t.value)
        P += [int(p[h]) for h in range(t.value)]
    return dict(mx=mx, my=my, qlen=qlen, P=np.array(P + [0], np.uint64), table=table, names=[b"chr0"], lens=np.array([200000], np.uint32), max_occ=max_occ, qname=None)


@pytest.mark.parametrize("flag", [0, FOR_ONLY])
def test_seed_and_window_batches_in_heap_order(dup, refheap, flag):  # noqa: F811
    D = dup
    ctx, idx = D["ctx"], D["idx"]
    L = gpu.lib()
    L.wm_index_get.restype = C.POINTER(C.c_uint64)
    L.wm_index_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]
    rng = np.random.default_rng(7)
    seqs = [np.ascontiguousarray(D["codes"][i]) for i in range(0, 200)]          # 200 whole reads, one job each
    minis = [W.o_sketch(bytes(s), 50, 15, rid=0) for s in seqs]
    nm = np.array([len(m[0]) for m in minis], np.int32)
    moff = np.concatenate([[0], np.cumsum(nm)[:-1]]).astype(np.uint64)
    allm = np.zeros((int(nm.sum()), 2), np.uint64)
    allm[:, 0] = np.concatenate([m[0] for m in minis]); allm[:, 1] = np.concatenate([m[1] for m in minis])
    qlen = np.array([len(s) for s in seqs], np.int32)
    max_occ = 200
    exp, pres = [], []
    n_tied = n_other_order = 0
    for j in range(len(seqs)):
        c = _job_case(L, idx, minis[j][0], minis[j][1], int(qlen[j]), max_occ)
        ex, ey, rep = ref_heap_list(refheap, c, flag, None)
        exp.append((ex, ey, rep))
        rx, ry, _ = _collect_seed_hits(c, flag, None)
        rx, ry = W.o_radix_sort_128x(rx, ry)                                     # what --heap-sort=no hands to the chain fill
        n_tied += has_tie(ex)
        n_other_order += not (np.array_equal(rx, ex) and np.array_equal(ry, ey))
        n_pre = 5 if j % 4 == 3 and len(ex) else 0                               # every fourth job: handed-in anchors, some on the x of seeded ones (src/map.c:818-833)
        px = ex[rng.integers(0, max(1, len(ex)), n_pre)] if n_pre else np.zeros(0, np.uint64)
        py = (rng.integers(0, int(qlen[j]), n_pre).astype(np.uint64) | np.uint64(15 << 32))
        o = np.argsort(px, kind="stable")
        pres.append((px[o], py[o]))
    assert n_tied >= 60 and n_other_order >= 40, (n_tied, n_other_order)          # the cases are worth something: a library that ignores the bit fails on them
    cap = sum(len(e[0]) for e in exp) * 2 + 4096
    out, ooff, na, rl = ctx.seed_batch_keyed(allm, moff, nm, qlen, None, max_occ, flag | HEAP, cap)
    for j, (ex, ey, rep) in enumerate(exp):
        g = out[int(ooff[j]):int(ooff[j]) + int(na[j])]
        assert na[j] == len(ex) and rl[j] == rep, (j, na[j], len(ex))
        assert np.array_equal(g[:, 0], ex) and np.array_equal(g[:, 1], ey), j
    J = np.zeros(len(seqs), gpu.WINDOW_JOB)
    J["seq_off"] = -1; J["len"] = qlen; J["stage_off"] = np.concatenate([[0], np.cumsum(qlen)[:-1]]); J["gap_scale"] = 1.0
    for k_, v in PAR.items():
        J[k_] = v
    J["n_pre"] = [len(p[0]) for p in pres]
    J["pre_off"] = np.concatenate([[0], np.cumsum([len(p[0]) for p in pres])[:-1]])
    pre = np.zeros((sum(len(p[0]) for p in pres) + 1, 2), np.uint64)
    pre[:-1, 0] = np.concatenate([p[0] for p in pres]); pre[:-1, 1] = np.concatenate([p[1] for p in pres])
    res, up, ap = ctx.window_batch_dust(J, None, np.concatenate(seqs), pre, max_occ, flag | HEAP, 0, cap, cap)
    n_chains = 0
    for j, (ex, ey, rep) in enumerate(exp):
        ox, oy = np.concatenate([pres[j][0], ex]), np.concatenate([pres[j][1], ey])
        if len(pres[j][0]):
            ox, oy = W.o_radix_sort_128x(ox, oy)                                 # :833, the seeded part in heap order as its input
        eu, evx, evy = W.o_chain_dp(ox, oy, **PAR) if len(ox) else (np.zeros(0, np.uint64),) * 3
        r = res[j]
        assert r["n_anchors"] == len(ox) and r["rep_len"] == rep and r["n_u"] == len(eu) and r["n_v"] == len(evx), (j, r)
        assert np.array_equal(up[r["u_off"]:r["u_off"] + r["n_u"]], eu), j
        a = ap[r["a_off"]:r["a_off"] + r["n_v"]]
        assert np.array_equal(a[:, 0], evx) and np.array_equal(a[:, 1], evy), j
        n_chains += len(eu)
    assert n_chains >= 150


def test_seeded_parts_beyond_the_lds_class(dup, refheap):  # noqa: F811
    """two jobs of more than 4 096 seeded anchors in both ops (the workgroup's sort in global memory, the heap in arena scratch): the 20 long duplicated reads
    in a row — equal x, replayed — and 150 kb of the contig itself, sorted only; the second with handed-in anchors (the union sort of src/map.c:833)"""
    D = dup
    ctx, idx = D["ctx"], D["idx"]
    L = gpu.lib()
    L.wm_index_get.restype = C.POINTER(C.c_uint64)
    L.wm_index_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]
    ref = synth.make_reference(1, 200000, 201)[0]
    seqs = [np.ascontiguousarray(np.concatenate(D["codes"][200:220])), np.ascontiguousarray(ref[20000:170000])]
    minis = [W.o_sketch(bytes(s), 50, 15, rid=0) for s in seqs]
    nm = np.array([len(m[0]) for m in minis], np.int32)
    moff = np.concatenate([[0], np.cumsum(nm)[:-1]]).astype(np.uint64)
    allm = np.zeros((int(nm.sum()), 2), np.uint64)
    allm[:, 0] = np.concatenate([m[0] for m in minis]); allm[:, 1] = np.concatenate([m[1] for m in minis])
    qlen = np.array([len(s) for s in seqs], np.int32)
    max_occ = 200
    exp = []
    for j in range(2):
        exp.append(ref_heap_list(refheap, _job_case(L, idx, minis[j][0], minis[j][1], int(qlen[j]), max_occ), 0, None))
    assert min(len(e[0]) for e in exp) > 4096 and has_tie(exp[0][0]), [len(e[0]) for e in exp]
    cap = sum(len(e[0]) for e in exp) * 2 + 4096
    out, ooff, na, rl = ctx.seed_batch_keyed(allm, moff, nm, qlen, None, max_occ, HEAP, cap)
    for j, (ex, ey, rep) in enumerate(exp):
        g = out[int(ooff[j]):int(ooff[j]) + int(na[j])]
        assert na[j] == len(ex) and rl[j] == rep, (j, na[j], len(ex))
        assert np.array_equal(g[:, 0], ex) and np.array_equal(g[:, 1], ey), j
    rng = np.random.default_rng(9)
    px = np.sort(exp[1][0][rng.integers(0, len(exp[1][0]), 7)])
    py = rng.integers(0, int(qlen[1]), 7).astype(np.uint64) | np.uint64(15 << 32)
    J = np.zeros(2, gpu.WINDOW_JOB)
    J["seq_off"] = -1; J["len"] = qlen; J["stage_off"] = [0, int(qlen[0])]; J["gap_scale"] = 1.0
    for k_, v in PAR.items():
        J[k_] = v
    J["n_pre"] = [0, 7]
    pre = np.zeros((8, 2), np.uint64)
    pre[:7, 0] = px; pre[:7, 1] = py
    res, up, ap = ctx.window_batch_dust(J, None, np.concatenate(seqs), pre, max_occ, HEAP, 0, cap, cap)
    for j, (ex, ey, rep) in enumerate(exp):
        ox, oy = (ex, ey) if j == 0 else W.o_radix_sort_128x(np.concatenate([px, ex]), np.concatenate([py, ey]))
        eu, evx, evy = W.o_chain_dp(ox, oy, **PAR)
        r = res[j]
        assert r["n_anchors"] == len(ox) and r["rep_len"] == rep and r["n_u"] == len(eu) and r["n_v"] == len(evx), (j, r)
        assert len(eu) > 0 and np.array_equal(up[r["u_off"]:r["u_off"] + r["n_u"]], eu), j
        a = ap[r["a_off"]:r["a_off"] + r["n_v"]]
        assert np.array_equal(a[:, 0], evx) and np.array_equal(a[:, 1], evy), j


# ---- 6. end to end against the reference binary ---------------------------------------------------------------------------------------------
def _mapper_text(ctx, idx, flag, names, seqs):
    m = gpu.Mapper(ctx, idx, "map-ont", flag)
    m.set_threads(8, 0)
    text = m.map(names, seqs)[0]
    defined = parity.defined_names(names, m.rep_len_defined())
    m.close()
    return text, defined


@need_ref
@need_wm
def test_duplicated_reads_map_like_the_reference_with_heap_sort(dup):
    D = dup
    args = ["-t", "1", "-cx", "map-ont", "--heap-sort=yes", D["fa"], D["rq"]]
    want, _ = _run(REF_BIN, args)
    no, _ = _run(REF_BIN, ["-t", "1", "-cx", "map-ont", "--heap-sort=no", D["fa"], D["rs"]])
    yes_short, _ = _run(REF_BIN, ["-t", "1", "-cx", "map-ont", "--heap-sort=yes", D["fa"], D["rs"]])
    d0 = parity.diff_texts(yes_short, no)
    print("reference --heap-sort=no against =yes on the 200 short reads:", {k: d0[k] for k in ("reads", "hits", "mismatches")})
    assert d0["reads"] == 200 and d0["mismatches"] >= 50, d0                      # the option changes the reference's own output on at least 25 % of these reads
    text, defined = _mapper_text(D["ctx"], D["idx"], BASE | HEAP, D["names"], D["seqs"])
    d = parity.diff_texts(want, text, defined=defined)
    assert d["reads"] == 220 and d["mapq_compared"] >= 200 and d["mismatches"] == 0, d
    got, _ = _run(WM_BIN, ["-t", "4", "-c", "-x", "map-ont", "--heap-sort=yes", D["fa"], D["rq"]])
    d = parity.diff_texts(want, got)
    assert d["reads"] == 220 and d["mismatches"] == 0, d


# ---- 7. combinations --------------------------------------------------------------------------------------------------------------------------
@need_ref
@need_wm
@pytest.mark.parametrize("extra,n_min", [(["--for-only"], 90), (["-T", "10"], 190), (["-H"], 190)])      # (--for-only: records for the forward half of the reads)
def test_heap_sort_combined_with_other_seeding_options(dup, extra, n_min):
    D = dup
    args = ["-t", "4", "-cx", "map-ont", "--heap-sort=yes"] + extra + [D["fa"], D["rs"]]
    want, _ = _run(REF_BIN, args)
    other, _ = _run(REF_BIN, ["-t", "4", "-cx", "map-ont", "--heap-sort=no"] + extra + [D["fa"], D["rs"]])
    assert parity.diff_texts(want, other)["mismatches"] >= 10                     # the heap order matters under this option as well
    got, _ = _run(WM_BIN, args)
    d = parity.diff_texts(want, got)
    assert d["reads"] >= n_min and d["mismatches"] == 0, (extra, d)


@pytest.fixture(scope="module")
def selfmap():
    """reference = reads (test_selfmap_gpu's input, smaller): 60 reads of 12 kb + 60 of 4 kb at ~6x over 150 kb, half of them with a duplication planted"""
    tmp = tempfile.mkdtemp()
    ref = synth.make_reference(1, 150000, 51, repeat_frac=0.08)
    reads = synth.make_reads(ref, 40, 12000, 52, profile="ont")[0] + synth.make_reads(ref, 40, 4000, 53, profile="ont")[0] + synth.make_dup_reads(ref, 40, 55)
    order = np.random.default_rng(54).permutation(len(reads))
    seqs = [synth.codes_to_ascii(reads[i]) for i in order]
    names = [(b"r%d" % i, b"read_%04d" % i, b"r%d/ccs" % i, b"R%d" % i)[i % 4] for i in range(len(seqs))]
    fa = os.path.join(tmp, "reads.fa")
    _write(fa, names, seqs)
    return dict(tmp=tmp, fa=fa, names=names, seqs=seqs)


@need_ref
@need_wm
def test_heap_sort_with_X_reads_against_themselves(selfmap):
    A = selfmap
    args = ["-t", "4", "-X", "-cx", "map-ont", "--heap-sort=yes", A["fa"], A["fa"]]
    want, _ = _run(REF_BIN, args)
    other, _ = _run(REF_BIN, ["-t", "4", "-X", "-cx", "map-ont", "--heap-sort=no", A["fa"], A["fa"]])
    assert parity.diff_texts(want, other)["mismatches"] >= 1                      # (few records: the plain reads carry no duplication; 6 on this input)
    got, _ = _run(WM_BIN, args)
    d = parity.diff_texts(want, got)
    assert d["reads"] >= 60 and d["mismatches"] == 0, d
    ctx = gpu.Context(0, 8 << 30)
    idx = gpu.Index(A["fa"], None, k=15, w=50, n_threads=8)
    idx.upload(ctx)
    try:
        text, defined = _mapper_text(ctx, idx, BASE | gpu.MM_F_AVA | HEAP, A["names"], A["seqs"])
    finally:
        idx.close(); ctx.close()
    d = parity.diff_texts(want, text, defined=defined)
    assert d["reads"] >= 60 and d["mismatches"] == 0, d


@need_ref
@need_wm
def test_heap_sort_with_a_two_part_split_index(dup):
    D = dup
    tmp = tempfile.mkdtemp()
    ref2 = os.path.join(tmp, "ref2.fa")                                           # the contig in two halves: two index parts at -I 120k
    chr0 = open(D["fa"], "rb").read().split(b"\n")[1]
    _write(ref2, [b"chrA", b"chrB"], [chr0[:100000], chr0[100000:]])
    args = ["-t", "1", "-I", "120k", "--split-prefix", os.path.join(tmp, "sp"), "-cx", "map-ont", "--heap-sort=yes", ref2, D["rs"]]
    want, _ = _run(REF_BIN, args)
    other, _ = _run(REF_BIN, args[:5] + [os.path.join(tmp, "sq")] + args[6:8] + ["--heap-sort=no", ref2, D["rs"]])
    assert parity.diff_texts(want, other)["mismatches"] >= 10
    args[5] = os.path.join(tmp, "sp2")
    got, _ = _run(WM_BIN, args)
    d = parity.diff_texts(want, got)
    assert d["reads"] >= 190 and d["mismatches"] == 0, d


# ---- 8. golden fixture --------------------------------------------------------------------------------------------------------------------------
def test_mapper_matches_the_heap_sort_golden():
    spec = importlib.util.spec_from_file_location("make_golden_heap", os.path.join(E.HERE, "golden", "make_golden_heap.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    preset, fa, k, reads = G.inputs(tempfile.mkdtemp())
    ctx = gpu.Context(0, 8 << 30)
    idx = gpu.Index(fa, None, k=k, w=50, n_threads=8)
    idx.upload(ctx)
    try:
        m = gpu.Mapper(ctx, idx, preset, gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG | HEAP)
        _, hits, cigars, first = m.map(["read%d" % i for i in range(len(reads))], reads)
        m.close()
    finally:
        idx.close(); ctx.close()
    E.compare(G.NAME, hits, cigars, first, reads)

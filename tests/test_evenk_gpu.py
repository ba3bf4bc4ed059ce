"""GPU: an even k. (3) wm_sketch_batch against the oracle on the cases of tests/evenkcases.py — staged bytes, resident packed reads through a window job, one
200 000-base sequence on one wavefront; (4) the window call at k = 14 stage by stage against oracle sketch -> collect_seed_hits restated -> the oracle's sort ->
the oracle's chaining, plain, with -T, in heap order and on an -H index; (5) the device index build against the host build and the reference's index; (6) the
reference's CLI bound to the library with WM_EVEN_K=1 against the reference, and the in-process mapper against the host glue on oracle ops.
The oracle's sketch is pinned to the reference's at these k by tests/test_evenk_emu.py and tests/test_oracle_vs_ref.py."""
import ctypes as C
import os
import tempfile

import numpy as np
import pytest

import evenkcases as EK
import e2e_common as E
import sdustcases as S
import wmtest as W
from winnowmap_amd import build, gpu, parity, synth
from test_aux_gpu import M128
from test_selfmap_gpu import _run, _write, REF_BIN, WM_BIN, need_ref, need_wm, BASE
from test_window_gpu import expected_seeds
from test_sdust_emu import ref_sdust  # noqa: F401  (a fixture)
from test_heapseed_emu import ref_heap_list, refheap, _Tab  # noqa: F401  (refheap: a fixture)

pytestmark = pytest.mark.gpu
PAR = dict(max_dist_x=5000, min_dist_x=1000, max_dist_y=5000, bw=500, max_skip=25, max_iter=5000, min_cnt=3, min_sc=40)


def _bind(L):
    L.wm_sketch_batch.argtypes = [C.c_void_p, C.c_int, W.u8p, C.c_size_t, W.u64p, W.i32p, C.c_void_p, C.c_size_t, W.u64p, W.i32p]
    L.wm_sketch_set_filter.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_uint32, C.c_int, C.c_int]
    L.wm_index_get.restype = C.POINTER(C.c_uint64)
    L.wm_index_get.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(C.c_int)]
    L.wm_last_aux_ms.restype = C.c_float
    L.wm_last_aux_ms.argtypes = [C.c_void_p]
    return L


def _sketch_batch(L, ctx, seqs):
    n = len(seqs)
    lens = np.array([len(s) for s in seqs], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    flat = np.concatenate(seqs)
    out = np.zeros(int(lens.sum()) + n, M128)
    ooff = np.zeros(n, np.uint64)
    cnt = np.zeros(n, np.int32)
    assert L.wm_sketch_batch(ctx._h, n, flat, flat.nbytes, offs, lens, out.ctypes.data, len(out), ooff, cnt) == 0, L.wm_last_error()
    return [out[int(o):int(o) + int(c)] for o, c in zip(ooff, cnt)]


def _jobs(n):
    J = np.zeros(n, gpu.WINDOW_JOB)
    J["gap_scale"] = 1.0
    for k_, v in PAR.items():
        J[k_] = v
    return J


def _per_job(out):
    res, up, ap = out
    return [(int(r["n_anchors"]), int(r["rep_len"]), int(r["n_mini"]), up[int(r["u_off"]):int(r["u_off"]) + int(r["n_u"])].tobytes(),
             ap[int(r["a_off"]):int(r["a_off"]) + int(r["n_v"])].tobytes()) for r in res]


# ---- 3. the sketch --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w,k,hpc", [(w, k, 0) for w, k in EK.PAIRS] + [(10, 16, 1), (50, 14, 1)])
def test_sketch_batch_at_even_k_equals_the_oracle(w, k, hpc):
    L = _bind(gpu.lib())
    tmp = tempfile.mkdtemp()
    ref = EK.reference(5, 2, 40000, 30)
    fa, kf = tmp + "/ref.fa", tmp + "/rep.txt"
    synth.write_fasta(fa, ref)
    km, cnt = synth.repetitive_kmers(ref, k)
    synth.write_kmer_list(kf, km, cnt, k)
    bloom = W.o_bloom(km)
    ctx = gpu.Context(0, 2 << 30)
    idx = gpu.Index(fa, kf, k=k, w=w, hpc=bool(hpc))
    idx.upload(ctx)
    try:
        seqs = EK.make_cases(w, k)
        EK.assert_exercises_rule(seqs, k, bool(hpc))
        exp = [W.o_sketch(bytes(s), w, k, rid=0, bloom=bloom, hpc=bool(hpc)) for s in seqs]
        got = _sketch_batch(L, ctx, seqs)
        for i, (g, (ex, ey)) in enumerate(zip(got, exp)):
            assert len(g) == len(ex) and np.array_equal(g["x"], ex) and np.array_equal(g["y"], ey), (i, len(seqs[i]), len(g), len(ex))
        assert sum(len(e[0]) for e in exp) > 100 and len(exp[-1][0]) == 0                 # (the last case: all (AT), not one minimizer)
        # the same bases as resident packed reads, through window jobs: every sequence staged and resident, job for job the same counts, chains and anchors
        flat = np.concatenate(seqs)
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])[:-1]])
        ctx.reads_upload(flat)
        J = _jobs(2 * len(seqs))
        for i, s in enumerate(seqs):
            J[2 * i]["seq_off"], J[2 * i]["stage_off"], J[2 * i]["len"] = -1, int(off[i]), len(s)
            J[2 * i + 1]["seq_off"], J[2 * i + 1]["len"] = int(off[i]), len(s)
        out = ctx.window_batch_dust(J, None, flat, np.zeros((1, 2), np.uint64), 50, 0, 0, 1 << 20, 1 << 22)
        pj = _per_job(out)
        for i in range(len(seqs)):
            assert pj[2 * i][2] == len(exp[i][0]) and pj[2 * i + 1] == pj[2 * i], (i, len(seqs[i]), pj[2 * i][:3], pj[2 * i + 1][:3], len(exp[i][0]))
    finally:
        idx.close(); ctx.close()


def test_sketch_of_200_000_bases_on_one_wavefront():
    """a sequence beyond WM_SKETCH_LONG with an (AT)5000 stretch inside: at k = 14 it stays on one wavefront (the chunked sketch cuts in position space), at
    k = 15 it is sketched chunk by chunk. Both equal the oracle; the kernel times are printed (DESIGN.md records them)."""
    L = _bind(gpu.lib())
    rng = np.random.default_rng(14)
    s = synth.random_codes(200000, rng)
    s[90000:100000] = np.tile(np.array([0, 3], np.uint8), 5000)
    s[150000:150003] = 4
    s[95000:95002] = 4                                     # (the array keeps its phase behind the N: every step there is skipped while l = 0)
    steps, skipped, low = EK.skip_stats(s, 14)
    assert skipped >= 9900 and low >= 10, (skipped, low)
    ctx = gpu.Context(0, 1 << 30)
    try:
        for k in (14, 15):
            assert L.wm_sketch_set_filter(ctx._h, None, 0, 0, 0, 0, k, 50) == 0, L.wm_last_error()
            g = _sketch_batch(L, ctx, [s])[0]
            ms = L.wm_last_aux_ms(ctx._h)
            ex, ey = W.o_sketch(bytes(s), 50, k, rid=0)
            assert len(g) == len(ex) and np.array_equal(g["x"], ex) and np.array_equal(g["y"], ey), (k, len(g), len(ex))
            print("sketch of 200 000 bases, w = 50, k = %d: %d minimizers, kernel %.3f ms" % (k, len(ex), ms))
    finally:
        ctx.close()


# ---- 4. the window call -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def win14():
    """a 2 x 150-kb reference with planted microsatellites, a -W list for k = 14; ~40 jobs of 500 - 12 000 bases: reads, their windows, stage-2 copies of reads
    with the mapped stretches masked by N, some with handed-in anchors"""
    tmp = tempfile.mkdtemp()
    ref = EK.reference(21, 2, 150000, 120)
    fa, kf = tmp + "/ref.fa", tmp + "/rep.txt"
    synth.write_fasta(fa, ref)
    km, cnt = synth.repetitive_kmers(ref, 14)
    synth.write_kmer_list(kf, km, cnt, 14)
    rng = np.random.default_rng(22)
    seqs = []
    for n, ln_ in ((10, 12000), (8, 4000), (8, 1500), (6, 500)):
        seqs += synth.make_reads(ref, n, ln_, 23 + ln_, profile="ont")[0]
    for r in seqs[:4]:                                     # stage-2 copies: everything but a few stretches masked
        m = np.full(len(r), 4, np.uint8)
        for _ in range(3):
            p, n = int(rng.integers(0, len(r) - 1500)), int(rng.integers(200, 1500))
            m[p:p + n] = r[p:p + n]
        seqs.append(m)
    for _ in range(4):                                     # windows over the planted arrays themselves, with an N
        c = ref[int(rng.integers(0, 2))]
        p = int(rng.integers(0, len(c) - 3000))
        s = c[p:p + 3000].copy()
        s[1000:1200] = np.tile(np.array([1, 2], np.uint8), 100)
        s[1100:1102] = 4                                   # (two bases: the array keeps its phase, every step behind the N is skipped while l = 0)
        seqs.append(s)
    seqs = [np.ascontiguousarray(s, np.uint8) for s in seqs]
    assert len(seqs) == 40 and min(len(s) for s in seqs) >= 500 and max(len(s) for s in seqs) <= 12000
    EK.assert_exercises_rule(seqs, 14)
    return dict(tmp=tmp, fa=fa, kf=kf, ref=ref, bloom=W.o_bloom(km), seqs=seqs)


def _heap_case(L, idx, mx, my, qlen, max_occ):
    t = C.c_int()
    P, table = [], _Tab()
    for x in mx:
        key = int(x) >> 8
        if key in table:
            continue
        p = L.wm_index_get(idx._h, key, C.byref(t))
        table[key] = (len(P), t.value)
        P += [int(p[h]) for h in range(t.value)]
    return dict(mx=mx, my=my, qlen=qlen, P=np.array(P + [0], np.uint64), table=table, names=[b"s0", b"s1"], lens=np.array([150000, 150000], np.uint32), max_occ=max_occ, qname=None)


@pytest.mark.parametrize("mode", ["plain", "dust", "heap", "hpc"])
def test_window_batch_at_k14_stage_by_stage(win14, mode, request):
    D = win14
    if mode in ("dust", "heap") and not W.have_ref():
        pytest.skip("oracle/_ref not built")
    L = _bind(gpu.lib())
    hpc = mode == "hpc"
    ctx = gpu.Context(0, 4 << 30)
    idx = gpu.Index(D["fa"], D["kf"], k=14, w=50, n_threads=8, hpc=hpc)
    idx.upload(ctx)
    L._wm_ref_index = None
    mi = None
    if W.have_ref() and not hpc:                           # the expectation's occurrence lists come from the reference's own index
        mi = W.ref().refshim_idx_build(D["fa"].encode(), D["kf"].encode(), 14, 50, 4)
        L._wm_ref_index = (W.ref(), mi)
    try:
        seqs = D["seqs"]
        rng = np.random.default_rng(5)
        T = 20 if mode == "dust" else 0
        flag = gpu.MM_F_HEAP_SORT if mode == "heap" else 0
        max_occ = 200
        iv_of = request.getfixturevalue("ref_sdust") if T else None
        heap = request.getfixturevalue("refheap") if flag else None
        exp, pres = [], []
        n_dropped = 0
        for j, s in enumerate(seqs):
            mx, my = W.o_sketch(bytes(s), 50, 14, rid=0, bloom=D["bloom"], hpc=hpc)
            if T:
                keep = S.restated_filter(mx, my, iv_of(s, T))
                n_dropped += len(mx) - len(keep)
                mx, my = mx[keep], my[keep]
            if flag:
                ex, ey, rep = ref_heap_list(heap, _heap_case(L, idx, mx, my, len(s), max_occ), 0, None)
            else:
                ex, ey, rep = expected_seeds(L, idx, s, mx, my, max_occ)
                ex, ey = W.o_radix_sort_128x(ex, ey) if len(ex) else (ex, ey)
            n_pre = int(rng.integers(1, 40)) if j % 5 == 2 else 0
            px = np.sort(rng.integers(0, 2, n_pre).astype(np.uint64) << np.uint64(63) | rng.integers(0, 2, n_pre).astype(np.uint64) << np.uint64(32) | rng.integers(0, 150000, n_pre).astype(np.uint64))
            if n_pre and len(ex):
                px[0] = ex[len(ex) // 2]                       # (one on the x of a seeded anchor)
                px = np.sort(px)
            py = rng.integers(0, len(s), n_pre).astype(np.uint64) | np.uint64(14 << 32)
            pres.append((px, py))
            ax, ay = np.concatenate([px, ex]), np.concatenate([py, ey])
            if n_pre:
                ax, ay = W.o_radix_sort_128x(ax, ay)
            exp.append((len(mx), ax, ay, rep))
        assert not T or n_dropped > 50, n_dropped
        flat = np.concatenate(seqs)
        off = np.concatenate([[0], np.cumsum([len(s) for s in seqs])[:-1]])
        ctx.reads_upload(flat)
        J = _jobs(len(seqs))
        for j, s in enumerate(seqs):
            J[j]["len"] = len(s)
            if j % 2:
                J[j]["seq_off"] = int(off[j])                  # resident
            else:
                J[j]["seq_off"], J[j]["stage_off"] = -1, int(off[j])
        J["n_pre"] = [len(p[0]) for p in pres]
        J["pre_off"] = np.concatenate([[0], np.cumsum([len(p[0]) for p in pres])[:-1]])
        pre = np.zeros((sum(len(p[0]) for p in pres) + 1, 2), np.uint64)
        pre[:-1, 0] = np.concatenate([p[0] for p in pres]); pre[:-1, 1] = np.concatenate([p[1] for p in pres])
        cap = sum(len(e[1]) for e in exp) * 2 + 4096
        res, up, ap = ctx.window_batch_dust(J, None, flat, pre, max_occ, flag, T, cap, cap)
        n_chains = 0
        for j, (n_mini, ax, ay, rep) in enumerate(exp):
            eu, evx, evy = W.o_chain_dp(ax, ay, **PAR) if len(ax) else (np.zeros(0, np.uint64),) * 3
            r = res[j]
            assert r["n_mini"] == n_mini and r["n_anchors"] == len(ax) and r["rep_len"] == rep, (mode, j, len(seqs[j]), r, n_mini, len(ax), rep)
            assert r["n_u"] == len(eu) and r["n_v"] == len(evx), (mode, j, r, len(eu), len(evx))
            assert np.array_equal(up[r["u_off"]:r["u_off"] + r["n_u"]], eu), (mode, j)
            a = ap[r["a_off"]:r["a_off"] + r["n_v"]]
            assert np.array_equal(a[:, 0], evx) and np.array_equal(a[:, 1], evy), (mode, j)
            n_chains += len(eu)
        assert n_chains >= 30, n_chains
    finally:
        if mi is not None:
            W.ref().refshim_idx_destroy(mi)
        L._wm_ref_index = None
        idx.close(); ctx.close()


# ---- 5. the device index build --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,hpc", [(14, False), (16, True)])
def test_device_index_build_at_even_k(k, hpc):
    L = _bind(gpu.lib())
    tmp = tempfile.mkdtemp()
    ref = EK.reference(31 + k, 2, 200000, 150)
    ref[1][5000:5040] = 4
    ref.append(np.tile(np.array([0, 3], np.uint8), 3000))              # (AT)n: not one minimizer
    ref.append(ref[0][:k + 3].copy())
    fa, kf = tmp + "/ref.fa", tmp + "/rep.txt"
    synth.write_fasta(fa, ref)
    km, cnt = synth.repetitive_kmers(ref[:2], k)
    synth.write_kmer_list(kf, km, cnt, k)
    host = gpu.Index(fa, kf, k=k, w=50, n_threads=8, hpc=hpc)
    hs, ha = host.export_arrays()
    c = gpu.Context(0, 2 << 30)
    try:
        dev, st = gpu.Index.build_on_device(c, fa, kf, k=k, w=50, n_threads=8, hpc=hpc)
        ds, da = dev.export_arrays()
        assert np.array_equal(hs, ds), (hs, ds)
        for a, b in zip(ha, da):
            assert np.array_equal(a, b)
        assert st["minimizers"] == host.n_minimizers and st["minimizers"] > 5000
        dev.upload(c)
        if W.have_ref():
            # against the reference's own index, by lookup, on every distinct minimizer the reference's sketch of the contigs yields
            R = W.ref()
            R.refshim_idx_build_flag.restype = C.c_void_p
            R.refshim_idx_build_flag.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
            mi = R.refshim_idx_build_flag(fa.encode(), kf.encode(), k, 50, 1 if hpc else 0, 4)
            if mi is not None:
                keys = set()
                for i, s in enumerate(ref):
                    rx, _ = W.r_sketch(mi, synth.codes_to_ascii(s), 50, k, rid=i, hpc=hpc)
                    keys.update(int(x) >> 8 for x in rx)
                buf = np.zeros(1 << 16, np.uint64)
                n_multi = 0
                for key in sorted(keys):
                    t = C.c_int()
                    p = L.wm_index_get(dev._h, key, C.byref(t))
                    n_ref = R.refshim_idx_get(mi, key, buf, len(buf))
                    assert t.value == n_ref and n_ref > 0, (key, t.value, n_ref)
                    assert np.array_equal(np.ctypeslib.as_array(p, shape=(n_ref,)), buf[:n_ref]), key
                    n_multi += n_ref > 1
                assert len(keys) > 5000 and n_multi >= 20, (len(keys), n_multi)
                R.refshim_idx_destroy(mi)
        dev.close()
    finally:
        host.close(); c.close()


# ---- 6. end to end ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def e2e():
    """a 300-kb reference with planted (AT)n / (CG)n arrays; 60 reads of 12 kb, 60 of 4 kb, a few of them twice"""
    tmp = tempfile.mkdtemp()
    ref = EK.reference(41, 2, 150000, 150)
    reads = synth.make_reads(ref, 60, 12000, 42, profile="ont")[0] + synth.make_reads(ref, 60, 4000, 43, profile="ont")[0]
    for i in range(0, len(reads), 6):                      # an array with two N inside, written into every sixth read: skips right behind an ambiguous base
        p = 300 + 17 * i
        reads[i][p:p + 60] = np.tile(np.array(((0, 3), (1, 2))[(i // 6) % 2], np.uint8), 30)
        reads[i][p + 30:p + 32] = 4
    reads += [reads[3], reads[70], reads[71]]
    order = np.random.default_rng(44).permutation(len(reads))
    seqs = [synth.codes_to_ascii(reads[i]) for i in order]
    names = [b"q%d" % i for i in range(len(seqs))]
    fa, rq = os.path.join(tmp, "ref.fa"), os.path.join(tmp, "reads.fa")
    _write(fa, [b"chrA", b"chrB"], [synth.codes_to_ascii(c) for c in ref])
    _write(rq, names, seqs)
    rx = os.path.join(tmp, "reads40.fa")                   # (-X: the reads against themselves, a subset — all-vs-all grows with the square)
    _write(rx, names[:40], seqs[:40])
    EK.assert_exercises_rule([reads[i] for i in order], 14)
    return dict(tmp=tmp, fa=fa, rq=rq, rx=rx, names=names, seqs=seqs, n=len(seqs))


ON = {"WM_EVEN_K": "1"}


def _swap_k(args, k):
    out = list(args)
    out[out.index("-k") + 1] = str(k)
    return out


@need_ref
@need_wm
@pytest.mark.parametrize("tag,extra", [("plain", ["-k", "14", "-cx", "map-ont"]), ("hpc", ["-k", "16", "-H", "-cx", "map-ont"]), ("dust", ["-k", "14", "-T", "20", "-cx", "map-ont"]),
                                       ("heap", ["-k", "14", "--heap-sort=yes", "-cx", "map-ont"]), ("asm20", ["-cx", "asm20", "-k", "18"])])
def test_bound_cli_at_even_k_prints_what_the_reference_prints(e2e, tag, extra):
    A = e2e
    args = ["-t", "4"] + extra + [A["fa"], A["rq"]]
    want, _ = _run(REF_BIN, args)
    odd, _ = _run(REF_BIN, _swap_k(args, 15))
    assert parity.diff_texts(want, odd)["mismatches"] >= 10                       # k matters: a library that ignored it would print something else
    got, _ = _run(WM_BIN, args, env=ON)
    d = parity.diff_texts(want, got)
    assert d["reads"] == A["n"] and d["hits"] >= 100 and d["mismatches"] == 0, (tag, d)


@need_ref
@need_wm
def test_bound_cli_at_even_k_reads_against_themselves(e2e):
    A = e2e
    args = ["-t", "4", "-k", "14", "-X", "-cx", "map-ont", A["rx"], A["rx"]]
    want, _ = _run(REF_BIN, args)
    odd, _ = _run(REF_BIN, _swap_k(args, 15))
    assert parity.diff_texts(want, odd)["mismatches"] >= 10
    got, _ = _run(WM_BIN, args, env=ON)
    d = parity.diff_texts(want, got)
    assert d["reads"] >= 20 and d["hits"] >= 40 and d["mismatches"] == 0, d


@need_ref
@need_wm
def test_bound_cli_at_even_k_two_part_split_index(e2e):
    A = e2e
    args = ["-t", "4", "-k", "14", "-I", "200k", "--split-prefix", os.path.join(A["tmp"], "sp"), "-cx", "map-ont", A["fa"], A["rq"]]
    want, _ = _run(REF_BIN, args)
    args[7] = os.path.join(A["tmp"], "sq")
    odd, _ = _run(REF_BIN, _swap_k(args, 15))
    assert parity.diff_texts(want, odd)["mismatches"] >= 10
    args[7] = os.path.join(A["tmp"], "sp2")
    got, _ = _run(WM_BIN, args, env=ON)
    d = parity.diff_texts(want, got)
    assert d["reads"] == A["n"] and d["hits"] >= 100 and d["mismatches"] == 0, d


def test_mapper_in_process_with_the_switch_and_without(e2e):
    """gpu.set_even_k(1): the mapper serves a k = 14 index and computes what the host glue computes on oracle ops; switched off, creation fails with "odd k"."""
    A = e2e
    H = C.CDLL(build.build_harness())
    H.h_index_build.restype = C.c_void_p
    H.h_index_build.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int]
    H.h_map.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_char_p, C.c_int, C.c_char_p, W.i32p, C.c_int, W.u32p, C.c_int64, C.POINTER(C.c_int64), W.u64p]
    pick = [i for i in range(A["n"]) if len(A["seqs"][i]) > 10000][:6] + [i for i in range(A["n"]) if len(A["seqs"][i]) < 10000][:10]
    names, seqs = [A["names"][i] for i in pick], [A["seqs"][i] for i in pick]
    ctx = gpu.Context(0, 8 << 30)
    idx = gpu.Index(A["fa"], None, k=14, w=50, n_threads=8)
    idx.upload(ctx)
    try:
        gpu.set_even_k(0)
        assert not gpu.even_k_enabled()
        with pytest.raises(gpu.WmError) as e:
            gpu.Mapper(ctx, idx, "map-ont", BASE)
        assert "odd k" in str(e.value) and "wm_set_even_k" in str(e.value)
        gpu.set_even_k(1)
        assert gpu.even_k_enabled()
        m = gpu.Mapper(ctx, idx, "map-ont", BASE)
        m.set_threads(8, 0)
        _, hits, cigars, first = m.map(names, seqs)
        m.close()
    finally:
        gpu.set_even_k(-1)
        idx.close(); ctx.close()
    h = H.h_index_build(A["fa"].encode(), b"", 14, 50, 4)
    assert h
    co_at = n_hits = 0
    for i, s in enumerate(seqs):
        ho = np.zeros(16 * 256, np.int32); co = np.zeros(2000000, np.uint32); nc = C.c_int64(); st = np.zeros(4, np.uint64)
        n = H.h_map(h, b"map-ont", BASE, s, len(s), names[i], ho, 256, co, len(co), C.byref(nc), st)
        a = hits[int(first[i]):int(first[i + 1])].copy(); b = ho[:16 * n].reshape(-1, 16).copy()
        assert len(a) == n, (i, len(s), len(a), n)
        E.mask_mapq(len(s), a, b)
        assert np.array_equal(a, b), (i, len(s))
        assert np.array_equal(cigars[co_at:co_at + nc.value], co[:nc.value]), (i, len(s))
        co_at += nc.value
        n_hits += n
    assert n_hits >= len(seqs) - 2

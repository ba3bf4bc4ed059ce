"""CPU: MM_F_EQX (--eqx, 0x4000000) on the host mapper driven by oracle-backed ops — mm_update_cigar_eqx (src/align.c:169-238; csrc/cigar_eqx.h) right behind every
scan, and deferred to one batched request per read (wm_set_eqx_device(1), served here by the default DeviceOps::eqx_batch), in all four combinations with the two
sibling switches. Against the reference's library and binary where oracle/_ref is built; and, independently of the reference, against the same run without the
flag: the = / X CIGAR collapses to exactly that CIGAR, it is what the rules give for the region's own bases, and both branches of the reference occur."""
import ctypes as C
import os
import subprocess
import tempfile
import numpy as np
import pytest
import wmtest as W
import e2e_common as E
import eqxcases as Q
from winnowmap_amd import build
from test_format_vs_ref import _mask

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_ref")
F_CIGAR, F_SAM, F_CG, F_CS, F_MD, F_EQX = 0x4, 0x8, 0x20, 0x40, 0x1000000, 0x4000000
GOLDENS = ["ont_short", "hifi", "asm20"]
CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    CODE[_c] = _i; CODE[_c + 32] = _i


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(build.build_harness())
    L.h_index_build_flag.restype = C.c_void_p
    L.h_index_build_flag.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.h_map.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_char_p, C.c_int, C.c_char_p, W.i32p, C.c_int, W.u32p, C.c_int64, C.POINTER(C.c_int64), W.u64p]
    L.h_map_text.restype = C.c_int64
    L.h_map_text.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), W.i32p, C.c_int, C.c_char_p, C.c_int64]
    for f in (L.wm_fix_stats, L.wm_extra_stats, L.wm_eqx_stats):
        f.argtypes = [W.u64p, C.c_int]; f.restype = None
    for f in (L.wm_set_fix_device, L.wm_set_extra_device, L.wm_set_eqx_device):
        f.argtypes = [C.c_int]; f.restype = None
    L.wm_eqx_device_enabled.restype = C.c_int
    return L


@pytest.fixture(autouse=True)
def switches_back(H):
    keys = ("WM_FIX_DEV", "WM_EXTRA_DEV", "WM_EQX_DEV")
    saved = {k: os.environ.pop(k, None) for k in keys}
    for f in (H.wm_set_fix_device, H.wm_set_extra_device, H.wm_set_eqx_device):
        f(-1)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        for f in (H.wm_set_fix_device, H.wm_set_extra_device, H.wm_set_eqx_device):
            f(-1)
        eqx_stats(H, True)


def eqx_stats(H, reset=False):
    out = np.zeros(6, np.uint64)
    H.wm_eqx_stats(out, 1 if reset else 0)
    return dict(zip(("deferred", "on_device", "on_host", "calls", "columns", "device_us"), (int(v) for v in out)))


def map_reads(H, h, preset, reads, flag):
    """-> per read: (hits [n, 16], [CIGAR of each hit])"""
    out = []
    for i, s in enumerate(reads):
        ho = np.zeros(16 * 256, np.int32); co = np.zeros(4000000, np.uint32); nc = C.c_int64(); st = np.zeros(4, np.uint64)
        n = H.h_map(h, preset.encode(), flag, s, len(s), ("read%d" % i).encode(), ho, 256, co, len(co), C.byref(nc), st)
        assert n >= 0 and nc.value <= len(co)
        hits = ho[:16 * n].reshape(-1, 16).copy()
        at, cigs = 0, []
        for r in hits:
            cigs.append(co[at:at + int(r[7])].copy()); at += int(r[7])
        assert at == nc.value
        out.append((hits, cigs))
    return out


@pytest.fixture(scope="module")
def RUNS(H):
    """computed once per golden: the index, the reads, the contigs, the run without the flag and the run with it (every switch unset)"""
    runs = {}
    for name in GOLDENS:
        tmp = tempfile.mkdtemp()
        preset, fa, kf, k, reads = E.make_golden.inputs(name, tmp)
        h = H.h_index_build_flag(fa.encode(), (kf or "").encode(), k, 50, 0, 4)
        assert h
        contigs = [CODE[np.frombuffer(b"".join(rec.split(b"\n")[1:]), np.uint8)] for rec in open(fa, "rb").read().split(b">")[1:]]
        for f in (H.wm_set_fix_device, H.wm_set_extra_device, H.wm_set_eqx_device):
            f(0)
        plain = map_reads(H, h, preset, reads, F_CIGAR | F_CG)
        eqx = map_reads(H, h, preset, reads, F_CIGAR | F_CG | F_EQX)
        runs[name] = dict(h=h, preset=preset, fa=fa, kf=kf, k=k, reads=reads, contigs=contigs, plain=plain, eqx=eqx)
    return runs


def collapse(cig):
    """7 / 8 back to 0, neighbours of one code merged"""
    out = []
    for w in cig:
        op, ln = int(w) & 0xf, int(w) >> 4
        op = 0 if op in (7, 8) else op
        if out and out[-1][0] == op:
            out[-1][1] += ln
        else:
            out.append([op, ln])
    return [(op, ln) for op, ln in out]


def collapse_words(cig):
    return np.array([ln << 4 | op for op, ln in collapse(cig)], np.uint32)


def operands(run, i, hit):
    """the region's own bases, 0..4 codes: the query strand it aligned, the contig stretch"""
    rid, rs, re, qs, qe, rev = (int(v) for v in hit[:6])
    q = CODE[np.frombuffer(run["reads"][i], np.uint8)]
    if rev:
        q = np.where(q[::-1] < 4, 3 - q[::-1], 4).astype(np.uint8)
        qs, qe = len(q) - qe, len(q) - qs
    return q[qs:qe], run["contigs"][rid][rs:re]


@pytest.mark.parametrize("name", GOLDENS)
def test_the_eqx_cigars_are_what_the_rules_give_for_the_regions_own_bases_and_both_branches_occur(RUNS, name):
    run = RUNS[name]
    n_branch = [0, 0]
    for i, ((h0, c0), (h1, c1)) in enumerate(zip(run["plain"], run["eqx"])):
        a, b = h0.copy(), h1.copy()
        a[:, 7] = b[:, 7] = 0                                                 # the op count is what changes; every other hit column stays
        assert np.array_equal(a, b), (name, i)
        for hit, plain, eqx in zip(h0, c0, c1):
            if not len(plain):
                assert not len(eqx)
                continue
            # collapsing 7 / 8 back to 0 and merging gives exactly the CIGAR of the run without the flag
            assert collapse(eqx) == collapse(plain), (name, i, hit[:6].tolist())
            assert not any((int(w) & 0xf) == 0 for w in eqx), (name, i, "an M op survived")
            q, t = operands(run, i, hit)
            want, in_place = Q.restated(plain, q, t)
            assert np.array_equal(eqx, want), (name, i, hit[:6].tolist(), in_place)
            n_branch[in_place] += 1
            if not in_place:          # in the rewrite branch every = column is equal and every X column unequal (the in-place branch relabels without looking)
                qo = to = 0
                for w in eqx:
                    op, ln = int(w) & 0xf, int(w) >> 4
                    if op == 7:
                        assert np.array_equal(q[qo:qo + ln], t[to:to + ln])
                    elif op == 8:
                        assert not (q[qo:qo + ln] == t[to:to + ln]).any()
                    qo += ln if op in (7, 8, 1) else 0; to += ln if op in (7, 8, 2, 3) else 0
                assert qo == len(q) and to == len(t)
    assert n_branch[0] > 0, (name, n_branch)
    run["n_branch"] = n_branch


def test_both_branches_of_the_reference_occurred_over_the_goldens(RUNS, H):
    """the goldens' reads carry errors, so their regions take the rewrite branch; exact copies of the reference take the in-place one (src/align.c:195-201)"""
    run = RUNS["hifi"]
    exact = [bytes(b"ACGT"[c] for c in run["contigs"][0][p:p + 3000]) for p in (1000, 30000)]
    got = map_reads(H, run["h"], run["preset"], exact, F_CIGAR | F_CG | F_EQX)
    n_in_place = n_rewrite = 0
    for i, (hits, cigs) in enumerate(got):
        for hit, cig in zip(hits, cigs):
            if len(cig):
                q, t = operands(dict(run, reads=exact), i, hit)
                n_in_place += Q.restated(collapse_words(cig), q, t)[1]
    for name in GOLDENS:
        for (h1, c1) in RUNS[name]["eqx"]:
            n_rewrite += sum(1 for cig in c1 if any((int(w) & 0xf) == 8 for w in cig))
    assert n_in_place >= 2 and n_rewrite > 0, (n_in_place, n_rewrite)
    assert text_of(got[0][1][0]) == "3000="


def text_of(cig):
    return "".join("%d%s" % (int(w) >> 4, "MIDNSHP=XB"[int(w) & 0xf]) for w in cig)


@pytest.mark.parametrize("fix,extra", [(0, 0), (0, 1), (1, 0), (1, 1)])
@pytest.mark.parametrize("name", GOLDENS)
def test_deferred_through_the_default_eqx_batch_gives_the_same_in_all_four_combinations(H, RUNS, name, fix, extra):
    run = RUNS[name]
    H.wm_set_fix_device(fix); H.wm_set_extra_device(extra)
    for on in (0, 1):
        H.wm_set_eqx_device(on)
        assert H.wm_eqx_device_enabled() == on
        eqx_stats(H, True)
        got = map_reads(H, run["h"], run["preset"], run["reads"], F_CIGAR | F_CG | F_EQX)
        st = eqx_stats(H)
        for i, ((h0, c0), (h1, c1)) in enumerate(zip(run["eqx"], got)):
            assert np.array_equal(h0, h1), (name, fix, extra, on, i)
            assert len(c0) == len(c1) and all(np.array_equal(x, y) for x, y in zip(c0, c1)), (name, fix, extra, on, i)
        if on:      # the oracle-backed ops have no device form: the default served every deferred region on the host
            assert st["deferred"] > 0 and st["on_host"] == st["deferred"] and st["on_device"] == 0 and st["calls"] == 0, st
            assert st["deferred"] >= sum(int((h[:, 7] > 0).sum()) for h, _ in got)
        else:
            assert not any(st.values()), st
    # without the flag the switch does nothing
    H.wm_set_eqx_device(1)
    eqx_stats(H, True)
    got = map_reads(H, run["h"], run["preset"], run["reads"][:3], F_CIGAR | F_CG)
    assert not any(eqx_stats(H).values())
    for (h0, c0), (h1, c1) in zip(run["plain"], got):
        assert np.array_equal(h0, h1) and all(np.array_equal(x, y) for x, y in zip(c0, c1))


def test_the_switch_overrides_the_environment(H):
    os.environ["WM_EQX_DEV"] = "1"
    H.wm_set_eqx_device(0)
    assert not H.wm_eqx_device_enabled()
    H.wm_set_eqx_device(-1)
    assert H.wm_eqx_device_enabled()
    os.environ["WM_EQX_DEV"] = "0"
    assert not H.wm_eqx_device_enabled()


@pytest.mark.skipif(not W.have_ref(), reason="oracle/_ref not built")
@pytest.mark.parametrize("name", GOLDENS)
def test_host_mapper_with_the_flag_equals_the_references_library(H, RUNS, name):
    R = W.ref()
    run = RUNS[name]
    mi = R.refshim_idx_build(run["fa"].encode(), (run["kf"] or "").encode(), run["k"], 50, 4)
    opt = R.refshim_mapopt(run["preset"].encode(), F_CIGAR | F_CG | F_EQX, mi)
    n_x = 0
    for i, (s, (hits, cigs)) in enumerate(zip(run["reads"], run["eqx"])):
        rh = np.zeros(16 * 256, np.int32); rc = np.zeros(4000000, np.uint32); rnc = C.c_int64()
        rn = R.refshim_map(mi, opt, s, len(s), ("read%d" % i).encode(), rh, 256, rc, len(rc), C.byref(rnc))
        assert rn == len(hits), (name, i, rn, len(hits))
        a = hits.copy(); b = rh[:16 * rn].reshape(-1, 16).copy()
        E.mask_mapq(len(s), a, b)
        assert np.array_equal(a, b), (name, i, a.tolist(), b.tolist())                 # all hit columns
        ours = np.concatenate(cigs + [np.zeros(0, np.uint32)])
        assert rnc.value == len(ours) and np.array_equal(ours, rc[:rnc.value]), (name, i)
        n_x += int(((ours & 0xf) == 8).sum())
    assert n_x > 0


@pytest.mark.skipif(not os.path.exists(REF_BIN), reason="oracle/_ref/winnowmap_ref not built")
@pytest.mark.parametrize("opts,flag,sam", [(["-c"], F_CG, False), (["-a"], F_SAM, True), (["-c", "--cs"], F_CG | F_CS, False), (["-a", "--MD"], F_SAM | F_MD, True)])
@pytest.mark.parametrize("dev", [0, 1])
def test_text_with_the_flag_equals_winnowmap_ref_eqx(H, RUNS, opts, flag, sam, dev):
    run = RUNS["ont_short"]
    reads = run["reads"][:8]
    tmp = tempfile.mkdtemp()
    rq = os.path.join(tmp, "reads.fa")
    with open(rq, "wb") as f:
        for i, s in enumerate(reads):
            f.write(b">read%d\n" % i + s + b"\n")
    cmd = [REF_BIN, "-t", "2"] + (["-W", run["kf"]] if run["kf"] else []) + ["-x", run["preset"], "--eqx"] + opts + [run["fa"], rq]
    ref_txt = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout.decode()
    n = len(reads)
    order = sorted(range(n), key=lambda i: (len(reads[i]), i), reverse=True)
    names = (C.c_char_p * n)(*[b"read%d" % i for i in order])
    seqs = (C.c_char_p * n)(*[reads[i] for i in order])
    lens = np.array([len(reads[i]) for i in order], np.int32)
    buf = C.create_string_buffer(64 << 20)
    H.wm_set_eqx_device(dev)
    m = H.h_map_text(run["h"], run["preset"].encode(), F_CIGAR | F_EQX | flag, n, names, seqs, lens, 2, buf, len(buf))
    assert m >= 0
    a = [x for x in (_mask(l, sam) for l in ref_txt.splitlines()) if x is not None and not x.startswith("@")]
    b = [x for x in (_mask(l, sam) for l in buf.raw[:m].decode().splitlines()) if x is not None]
    assert len(a) == len(b) > 0 and any("X" in (x.split("\t")[5] if sam else x) for x in a)
    for x, y in zip(a, b):
        assert x == y, "\nref : %s\nours: %s" % (x[:600], y[:600])

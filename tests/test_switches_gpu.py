"""GPU: the mapper with ALL FIVE opt-in device passes on at once — wm_set_fix_device, wm_set_extra_device, wm_set_eqx_device, wm_set_cs_device, wm_set_ll_device — i.e. the glue
of csrc/wm_mapper.hip that feeds the kernels (pack_final, call_retry, run_split, batch_or_rest and the CallOps overrides), which no emulator reaches. (a) all on against all
off and the goldens under six flag sets, the cs pass reading the = / X CIGARs the eqx pass has just written on the device, with the accounts of all five; (b) every one of the
32 subsets of the switches; (c) two mapping calls in flight; (d) the file loop; (e) reads that are NOT resident (WM_NO_RESIDENT: the byte slab of ksw_batch, the staged
sketch, and the host fall-back branch of every pass); (f) the bound command line with all five variables set."""
import ctypes as C
import os
import subprocess
import tempfile
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import wmtest as W
import e2e_common as E
from winnowmap_amd import gpu, synth, parity
from test_eqx_gpu import collapsed
from test_ll_gpu import inversion_input, splice_input

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_ref")
WM_BIN = os.path.join(ROOT, "oracle", "_ref", "winnowmap_wm")
SWITCHES = ("fix", "extra", "eqx", "cs", "ll")
BASE = gpu.MM_F_CIGAR | gpu.MM_F_OUT_CG
EQX, CS, CS_LONG, MD = gpu.MM_F_EQX, gpu.MM_F_OUT_CS, gpu.MM_F_OUT_CS_LONG, gpu.MM_F_OUT_MD
FLAGSETS = {"plain": 0, "eqx": EQX, "cs": CS, "eqx_cs": EQX | CS, "eqx_cslong": EQX | CS | CS_LONG, "eqx_md": EQX | MD}
GOLDENS = ("ont_short", "hifi")
# the inputs whose reads reach ksw_ll_i16: the inversion tests of the inversion reads, the end filter of the splice set, and two z-dropped fills of hifi (the host mapper
# over the oracle's operations files 2 jobs there: tests/test_switches_host.py counts the same way); no fill of ont_short z-drops
LL_INPUTS = ("inversion", "splice", "hifi")


def set_all(on):
    for s in SWITCHES:
        getattr(gpu, "set_%s_device" % s)(on)


def set_mask(mask):
    for k, s in enumerate(SWITCHES):
        getattr(gpu, "set_%s_device" % s)(mask >> k & 1)


def stats(reset=False):
    return {s: getattr(gpu, "%s_stats" % s)(reset=reset) for s in SWITCHES}


@pytest.fixture(autouse=True)
def restore_switches():
    """all process-global: every test leaves the library's defaults behind"""
    try:
        yield
    finally:
        set_all(-1)
        stats(reset=True)


@pytest.fixture(scope="module")
def ctx():
    c = gpu.Context(0, 4 << 30)
    yield c
    c.close()


@pytest.fixture(scope="module")
def INPUTS(ctx):
    """one index per input, built once and uploaded whenever it is asked for: name -> dict(idx, preset, reads, names, fa, kf, k, w)"""
    made = {}
    tmp = tempfile.mkdtemp()

    def get(name):
        if name not in made:
            if name in GOLDENS:
                preset, fa, kf, k, reads = E.make_golden.inputs(name, tmp)
                w = 50
            else:
                preset, fa, k, w, reads = (inversion_input if name == "inversion" else splice_input)(tmp)
                kf = None
            idx = gpu.Index(fa, kf, k=k, w=w, n_threads=8)
            made[name] = dict(idx=idx, preset=preset, reads=reads, names=["read%d" % i for i in range(len(reads))], fa=fa, kf=kf, k=k, w=w)
        made[name]["idx"].upload(ctx)          # a context holds ONE uploaded index, the last one: whoever asks for an input maps on it next
        return made[name]
    yield get
    for d in made.values():
        d["idx"].close()


def same(a, b):
    return a[0] == b[0] and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(a[3], b[3])


def check_served_on_the_device(st, name, flag, text):
    """the accounts after an all-on run of resident reads"""
    for s in SWITCHES:
        assert st[s]["on_host"] == 0, (s, st[s])
    fx, ex, eq, cs, ll = (st[s] for s in SWITCHES)
    assert fx["deferred"] > 0 and fx["on_device"] + fx["early_on_host"] == fx["deferred"] and fx["calls"] > 0, fx
    # a region that an inversion test read was fixed early on the host: only its scan travels, as a request of the extra pass
    assert ex["deferred"] == fx["early_on_host"] and ex["on_device"] == ex["deferred"], (ex, fx)
    assert eq["on_device"] == eq["deferred"] and cs["on_device"] == cs["deferred"] and ll["on_device"] == ll["deferred"], (eq, cs, ll)
    assert (eq["deferred"] > 0) == bool(flag & EQX) and (cs["deferred"] > 0) == bool(flag & (CS | MD)) and (ll["deferred"] > 0) == (name in LL_INPUTS), (name, eq, cs, ll)
    if flag & (CS | MD):
        assert cs["deferred"] == text.count(b"\tMD:Z:" if flag & MD else b"\tcs:Z:")
    for s, acc in zip(SWITCHES, (fx, ex, eq, cs, ll)):          # a pass with nothing to do has not moved a counter
        if acc["deferred"] == 0:
            assert not any(acc.values()), (s, acc)
        else:
            assert acc["calls"] > 0, (s, acc)


def reference_mapper(run, flag):
    """the goldens' generator: the real reference through oracle/_ref, under the same flag"""
    R = W.ref()
    mi = R.refshim_idx_build(run["fa"].encode(), (run["kf"] or "").encode(), run["k"], run["w"], 4)
    opt = R.refshim_mapopt(run["preset"].encode(), flag, mi)
    hits, cigs, first = [], [], [0]
    for i, s in enumerate(run["reads"]):
        h = np.zeros(16 * 256, np.int32); c = np.zeros(4000000, np.uint32); nc = C.c_int64()
        n = R.refshim_map(mi, opt, s, len(s), ("read%d" % i).encode(), h, 256, c, len(c), C.byref(nc))
        hits.append(h[:16 * n].reshape(-1, 16).copy()); cigs.append(c[:nc.value].copy()); first.append(first[-1] + n)
    return np.concatenate(hits), np.concatenate(cigs), np.array(first, np.int64)


# ---- (a) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fl", list(FLAGSETS))
@pytest.mark.parametrize("name", GOLDENS + ("inversion", "splice"))
def test_all_five_on_give_what_all_five_off_give_and_the_device_served_every_request(ctx, INPUTS, name, fl):
    run = INPUTS(name)
    flag = BASE | FLAGSETS[fl]
    m = gpu.Mapper(ctx, run["idx"], run["preset"], flag)
    try:
        set_all(0)
        stats(reset=True)
        off = m.map(run["names"], run["reads"])
        assert not any(v for acc in stats().values() for v in acc.values())
        set_all(1)
        on = m.map(run["names"], run["reads"])
        st = stats()
    finally:
        m.close()
    text, hits, cigars, first = on
    assert same(on, off)
    assert (b"\tcs:Z:" in text) == bool(flag & CS) and (b"\tMD:Z:" in text) == bool(flag & MD)
    if flag & EQX:
        assert not ((cigars & 0xf) == 0).any() and ((cigars & 0xf) == 8).any()
    if name in GOLDENS:
        E.compare(name, *(collapsed(hits, cigars) if flag & EQX else (hits, cigars)), first, run["reads"])
    check_served_on_the_device(st, name, flag, text)
    if W.have_ref() and fl == "eqx_cs" and name in ("ont_short", "inversion"):
        rh, rc, rf = reference_mapper(run, flag)
        g, h = rh.copy(), hits.copy()
        for i, s in enumerate(run["reads"]):
            E.mask_mapq(len(s), g[int(rf[i]):int(rf[i + 1])], h[int(first[i]):int(first[i + 1])])
        assert np.array_equal(rf, first) and np.array_equal(g, h) and np.array_equal(rc, cigars)


@pytest.mark.parametrize("mask", [0b00001, 0b11011])
@pytest.mark.parametrize("name", GOLDENS + ("inversion", "splice"))
def test_the_fix_on_the_device_with_the_rewriting_left_to_the_host_gives_what_all_five_off_give(ctx, INPUTS, name, mask):
    """the fix alone, and all but the eqx pass: the = / X rewriting then runs on the host behind the device's fix, at the operands advanced by the shifts it reports"""
    run = INPUTS(name)
    m = gpu.Mapper(ctx, run["idx"], run["preset"], BASE | EQX | CS)
    try:
        set_all(0)
        off = m.map(run["names"], run["reads"])
        set_mask(mask)
        stats(reset=True)
        on = m.map(run["names"], run["reads"])
        st = stats()
    finally:
        m.close()
    assert same(on, off) and ((on[2] & 0xf) == 8).any()
    assert st["fix"]["on_device"] > 0 and st["fix"]["on_host"] == 0 and not any(st["eqx"].values()), st


# ---- (b) ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def SUBSETS():
    """one mapper for the 32 subsets, on a context of its own (a mapper keeps the resident reads of the context it maps on), and the all-off run they are held against"""
    c = gpu.Context(0, 1 << 30)
    tmp = tempfile.mkdtemp()
    preset, fa, k, w, reads = inversion_input(tmp)
    idx = gpu.Index(fa, None, k=k, w=w, n_threads=8)
    idx.upload(c)
    m = gpu.Mapper(c, idx, preset, BASE | EQX | CS)
    names = ["read%d" % i for i in range(len(reads))]
    set_all(0)
    base = m.map(names, reads)
    set_all(-1)
    yield m, names, reads, base
    m.close(); idx.close(); c.close()


@pytest.mark.parametrize("mask", range(32))
def test_every_subset_of_the_five_switches_gives_the_all_off_run(SUBSETS, mask):
    m, names, reads, base = SUBSETS
    set_mask(mask)
    stats(reset=True)
    got = m.map(names, reads)
    st = stats()
    assert same(got, base), mask
    assert base[0].count(b"\tcs:Z:") > 0 and ((base[2] & 0xf) == 8).any()
    on = {s: bool(mask >> k & 1) for k, s in enumerate(SWITCHES)}
    for s in SWITCHES:
        assert st[s]["on_host"] == 0, (mask, s, st[s])
        if s != "extra":
            assert (st[s]["deferred"] > 0) == on[s] and (st[s]["on_device"] > 0) == on[s], (mask, s, st[s])
    # the scan alone travels for every region when only its switch is on, and for the early-fixed regions when the fix travels too
    assert (st["extra"]["deferred"] > 0) == (on["extra"] or on["fix"]), (mask, st["extra"], st["fix"])
    if on["fix"]:
        assert st["fix"]["early_on_host"] > 0 and st["extra"]["deferred"] == st["fix"]["early_on_host"], (mask, st["fix"], st["extra"])
    assert st["extra"]["on_device"] == st["extra"]["deferred"]


# ---- (c) ----------------------------------------------------------------------------------------------------------------------------
def test_two_mapping_calls_in_flight_with_8_host_threads_give_the_same_with_all_five_on_and_off(ctx, INPUTS):
    run = INPUTS("inversion")
    reads = run["reads"][:4]
    m = gpu.Mapper(ctx, run["idx"], run["preset"], BASE | EQX | CS)
    m.set_threads(8, 1 << 30)
    halves = [(["a%d" % i for i in range(len(reads))], reads), (["b%d" % i for i in range(len(reads))], reads[::-1])]

    def both_slots():
        with ThreadPoolExecutor(2) as ex:
            fs = [ex.submit(m.map, halves[s][0], halves[s][1], True, s) for s in (0, 1)]
            return [f.result()[0] for f in fs]
    try:
        set_all(0)
        off = both_slots()
        set_all(1)
        stats(reset=True)
        on = both_slots()
        st = stats()
    finally:
        m.close()
    assert on == off and all(t.count(b"\tcs:Z:") >= len(reads) and b"=" in t for t in on)
    for s in SWITCHES:
        assert st[s]["on_host"] == 0 and st[s]["deferred"] > 0, (s, st[s])
    assert st["fix"]["calls"] >= 2 and st["eqx"]["calls"] >= 2 and st["cs"]["calls"] >= 2, st


# ---- (d) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["paf", "sam"])
def test_the_file_loop_writes_the_same_file_with_all_five_on_and_off(ctx, fmt):
    tmp = tempfile.mkdtemp()
    ref = synth.make_reference(1, 300000, 41, repeat_frac=0.05)
    fa = os.path.join(tmp, "ref.fa")
    synth.write_fasta(fa, ref, prefix="chr")
    reads = [synth.codes_to_ascii(r) for r in synth.make_reads(ref, 40, 3000, 42, profile="ont")[0]]
    rq = os.path.join(tmp, "reads.fa")
    with open(rq, "wb") as f:
        for i, s in enumerate(reads):
            f.write(b">read%d\n" % i + s + b"\n")
    idx = gpu.Index(fa, None, k=15, w=50, n_threads=8)
    idx.upload(ctx)
    m = gpu.Mapper(ctx, idx, "map-ont", gpu.MM_F_CIGAR | (gpu.MM_F_OUT_SAM if fmt == "sam" else gpu.MM_F_OUT_CG) | EQX | CS)
    m.set_threads(4, 1 << 30)
    K = 25000                                   # 120 kb of reads: five mini-batches over the file loop's two lanes
    files = []
    try:
        for on in (0, 1):
            set_all(on)
            stats(reset=True)
            outp = os.path.join(tmp, "out%d.%s" % (on, fmt))
            run = m.map_file(rq, outp, K)
            assert run["reads"] == len(reads) and run["batches"] >= 4, run
            files.append(open(outp, "rb").read())
        st = stats()
    finally:
        m.close()
        idx.close()
    assert files[1] == files[0] and files[0].count(b"\tcs:Z:") >= len(reads) - 2 and b"=" in files[0]
    for s in ("fix", "eqx", "cs"):
        assert st[s]["on_host"] == 0 and st[s]["on_device"] > 0 and st[s]["calls"] >= 4, (s, st[s])
    assert st["extra"]["on_host"] == 0 and st["ll"]["on_host"] == 0, st


# ---- (e) ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", GOLDENS)
def test_reads_that_are_not_resident_give_the_goldens_and_the_resident_run(ctx, INPUTS, monkeypatch, name):
    run = INPUTS(name)
    set_all(0)
    m = gpu.Mapper(ctx, run["idx"], run["preset"], BASE)
    try:
        res = m.map(run["names"], run["reads"])
    finally:
        m.close()
    monkeypatch.setenv("WM_NO_RESIDENT", "1")
    m = gpu.Mapper(ctx, run["idx"], run["preset"], BASE)
    try:
        non = m.map(run["names"], run["reads"])
    finally:
        m.close()
    E.compare(name, non[1], non[2], non[3], run["reads"])
    assert same(non, res) and len(non[1]) >= len(run["reads"]) - 2


@pytest.mark.parametrize("name", ["ont_short", "inversion"])
def test_with_reads_that_are_not_resident_every_pass_falls_back_to_the_host_and_gives_the_same(ctx, INPUTS, monkeypatch, name):
    run = INPUTS(name)
    flag = BASE | EQX | CS
    set_all(0)
    m = gpu.Mapper(ctx, run["idx"], run["preset"], flag)
    try:
        res = m.map(run["names"], run["reads"])
    finally:
        m.close()
    monkeypatch.setenv("WM_NO_RESIDENT", "1")
    m = gpu.Mapper(ctx, run["idx"], run["preset"], flag)
    try:
        set_all(1)
        stats(reset=True)
        non = m.map(run["names"], run["reads"])
        st = stats()
    finally:
        m.close()
    assert same(non, res) and non[0].count(b"\tcs:Z:") > 0 and ((non[2] & 0xf) == 8).any()
    for s in SWITCHES:
        assert st[s]["on_device"] == 0 and st[s]["calls"] == 0, (s, st[s])
    for s in ("eqx", "cs") + (("ll",) if name == "inversion" else ()):
        assert st[s]["on_host"] == st[s]["deferred"] > 0, (s, st[s])
    if name != "inversion":
        assert not any(st["ll"].values()), st["ll"]
    assert st["fix"]["on_host"] + st["fix"]["early_on_host"] == st["fix"]["deferred"] > 0, st["fix"]
    assert st["extra"]["on_host"] == st["extra"]["deferred"] == st["fix"]["early_on_host"], (st["extra"], st["fix"])
    assert (st["fix"]["early_on_host"] > 0) == (name == "inversion")


# ---- (f) ----------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def CLI_INPUT():
    """the input of tests/test_cs_gpu.py's command-line test, written once"""
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
    return fa, kf, rq


@pytest.mark.skipif(not (os.path.exists(REF_BIN) and os.path.exists(WM_BIN)), reason="oracle/_ref/winnowmap_ref / winnowmap_wm not built")
@pytest.mark.parametrize("fmt,tagopt", [("-cx", "--cs"), ("-ax", "--MD")])
def test_the_bound_cli_with_all_five_variables_set_prints_what_winnowmap_ref_prints(CLI_INPUT, fmt, tagopt):
    fa, kf, rq = CLI_INPUT
    env = dict(os.environ, WM_EXTRA_REPORT="1", **{"WM_%s_DEV" % s.upper(): "1" for s in SWITCHES})

    def run(binary, args):
        p = subprocess.run([binary] + args, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=600)
        assert p.returncode == 0, p.stderr.decode(errors="replace")[-2000:]
        return p.stdout, p.stderr
    args = ["-t", "4", "-W", kf, "--eqx", tagopt, fmt, "map-ont", fa, rq]
    want, got = run(REF_BIN, args)[0], run(WM_BIN, args)
    d = parity.diff_texts(want, got[0], sam=fmt == "-ax")
    assert d["reads"] >= 20 and d["hits"] >= 20 and d["mismatches"] == 0, (fmt, d)
    tag = b"\tMD:Z:" if tagopt == "--MD" else b"\tcs:Z:"
    assert got[0].count(tag) >= 20 and got[0].count(tag) == want.count(tag) and b"=" in got[0] and b"X" in got[0]
    # every switch was on, and the device served every request (WM_EXTRA_REPORT, host/wm_ops.cpp: an account with nothing deferred prints nothing)
    for acc in (b"fix", b"eqx", b"cs"):
        line = [l for l in got[1].splitlines() if l.startswith(b"[wm] " + acc + b": ")]
        assert len(line) == 1 and b" 0 on the host" in line[0], (acc, got[1][-800:])

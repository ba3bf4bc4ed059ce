"""CPU: the host mapper with ksw_ll_i16 filed as local-score requests (wm_set_ll_device(1): the inversion test of mm_test_zdrop, mm_align1_inv's placement and the
splice end filter go through the alignment queue of the batching hub, split off in front of ksw_batch / exts2_batch and served here by the default
DeviceOps::ll_batch, i.e. the host form) must give exactly what it gives with the switch off — hits, CIGARs and text — on reads with an inverted stretch and on a
splice-mode input, in every combination with the four sibling switches; wm_ll_stats counts what it did. With the switch off nothing is filed: the account stays zero
and the hub serves as many requests as before."""
import ctypes as C
import os
import tempfile
import numpy as np
import pytest
import wmtest as W
from winnowmap_amd import build, synth

NAMES = ("deferred", "on_device", "on_host", "calls", "cells", "device_us")
F_CIGAR, F_CG, F_CS, F_EQX = 0x4, 0x20, 0x40, 0x4000000
SIBLINGS = ("fix", "extra", "eqx", "cs")


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(build.build_harness())
    L.h_index_build_flag.restype = C.c_void_p
    L.h_index_build_flag.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.h_map.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_char_p, C.c_int, C.c_char_p, W.i32p, C.c_int, W.u32p, C.c_int64, C.POINTER(C.c_int64), W.u64p]
    L.h_map_text.restype = C.c_int64
    L.h_map_text.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int, C.POINTER(C.c_char_p), C.POINTER(C.c_char_p), W.i32p, C.c_int, C.c_char_p, C.c_int64]
    L.wm_ll_stats.argtypes = [W.u64p, C.c_int]; L.wm_ll_stats.restype = None
    for s in SIBLINGS + ("ll",):
        f = getattr(L, "wm_set_%s_device" % s)
        f.argtypes = [C.c_int]; f.restype = None
    L.wm_ll_device_enabled.restype = C.c_int
    return L


def stats(H, reset=False):
    out = np.zeros(6, np.uint64)
    H.wm_ll_stats(out, 1 if reset else 0)
    return dict(zip(NAMES, (int(v) for v in out)))


@pytest.fixture(autouse=True)
def switches_back(H):
    keys = ["WM_%s_DEV" % s.upper() for s in SIBLINGS + ("ll",)]
    saved = {k: os.environ.pop(k, None) for k in keys}
    sets = [getattr(H, "wm_set_%s_device" % s) for s in SIBLINGS + ("ll",)]
    for f in sets:
        f(-1)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        for f in sets:
            f(-1)
        stats(H, True)


def map_reads(H, h, preset, reads, flag=F_CIGAR | F_CG):
    """hits, CIGARs, first hit per read, and the hub's counts summed over the reads: batches, alignment requests, chain requests, sketch requests"""
    hits, cigs, first, hub = [], [], [0], np.zeros(4, np.uint64)
    for i, s in enumerate(reads):
        ho = np.zeros(16 * 256, np.int32); co = np.zeros(2000000, np.uint32); nc = C.c_int64(); st = np.zeros(4, np.uint64)
        n = H.h_map(h, preset.encode(), flag, s, len(s), ("read%d" % i).encode(), ho, 256, co, len(co), C.byref(nc), st)
        assert n >= 0
        hits.append(ho[:16 * n].reshape(-1, 16).copy()); cigs.append(co[:nc.value].copy()); first.append(first[-1] + n); hub += st
    return np.concatenate(hits), np.concatenate(cigs), np.array(first, np.int64), [int(v) for v in hub]


def map_text(H, h, preset, reads, flag, threads=2):
    n = len(reads)
    names = (C.c_char_p * n)(*[b"read%d" % i for i in range(n)])
    seqs = (C.c_char_p * n)(*reads)
    lens = np.array([len(r) for r in reads], np.int32)
    buf = C.create_string_buffer(32 << 20)
    m = H.h_map_text(h, preset.encode(), flag, n, names, seqs, lens, threads, buf, len(buf))
    assert m >= 0
    return buf.raw[:m].decode()


@pytest.fixture(scope="module")
def INPUTS(H):
    """computed once: the inversion reads of tests/test_fix_host.py (an inverted stretch in the middle of each read) and a splice-mode input, each with its index"""
    tmp = tempfile.mkdtemp()
    rng = np.random.default_rng(17)
    ref = synth.make_reference(1, 120000, 23, repeat_frac=0.0)
    fa = os.path.join(tmp, "inv.fa")
    synth.write_fasta(fa, ref)
    reads = []
    for i in range(6):
        p = int(rng.integers(2000, 90000))
        r = ref[0][p:p + 9000].copy()
        a = int(rng.integers(3000, 4000)); ln = int(rng.integers(600, 1500))
        r[a:a + ln] = synth.revcomp_codes(r[a:a + ln])
        for q in rng.integers(0, len(r), 90):
            r[q] = (r[q] + 1) % 4
        reads.append(synth.codes_to_ascii(r))
    inv = dict(preset="map-ont", reads=reads, h=H.h_index_build_flag(fa.encode(), b"", 15, 50, 0, 4))
    ref2 = synth.make_reference(2, 200000, 191, repeat_frac=0.05)
    tr = [synth.codes_to_ascii(r) for r in synth.make_transcripts(ref2, 16, 192)]
    fa2 = os.path.join(tmp, "splice.fa")
    synth.write_fasta(fa2, ref2)
    # (k = 9: an anchor of 9 bases weighs less than log(gap) + anchor_ext_shift across most gaps, so mm_fix_bad_ends_splice asks for scores; at k = 15 it takes a gap of
    # 8 kb, longer than any intron of this input, and the filter would never call ksw_ll_i16)
    spl = dict(preset="splice", reads=tr, h=H.h_index_build_flag(fa2.encode(), b"", 9, 25, 0, 4))
    assert inv["h"] and spl["h"]
    return {"inversion": inv, "splice": spl}


@pytest.mark.parametrize("name", ["inversion", "splice"])
def test_hits_cigars_and_text_with_the_switch_on_equal_those_with_it_off(H, INPUTS, name):
    run = INPUTS[name]
    stats(H, True)
    assert not H.wm_ll_device_enabled()                                    # off by default
    hits_d, cigs_d, first_d, hub_d = map_reads(H, run["h"], run["preset"], run["reads"])
    H.wm_set_ll_device(0)
    hits0, cigs0, first0, hub0 = map_reads(H, run["h"], run["preset"], run["reads"])
    text0 = map_text(H, run["h"], run["preset"], run["reads"], F_CIGAR | F_CG | F_CS)
    # the switch off, unset or set: nothing is filed, the account stays zero, and the hub serves what it served
    assert not any(stats(H).values()) and hub0 == hub_d
    assert np.array_equal(hits_d, hits0) and np.array_equal(cigs_d, cigs0)
    H.wm_set_ll_device(1)
    hits, cigs, first, hub = map_reads(H, run["h"], run["preset"], run["reads"])
    st = stats(H)
    assert np.array_equal(hits, hits0) and np.array_equal(cigs, cigs0) and np.array_equal(first, first0)
    # the oracle-backed ops have no device form: the default served every filed job on the host, through the alignment queue
    assert st["deferred"] > 0 and st["on_host"] == st["deferred"] and st["on_device"] == 0 and st["calls"] == 0 and st["cells"] == 0, st
    assert hub[1] == hub0[1] + st["deferred"] and hub[2:] == hub0[2:], (hub, hub0, st)
    stats(H, True)
    assert map_text(H, run["h"], run["preset"], run["reads"], F_CIGAR | F_CG | F_CS) == text0
    assert stats(H)["deferred"] == st["deferred"]                           # (the same jobs, whatever the team of workers)
    if name == "inversion":
        assert int((hits[:, 15] >> 1 & 1).sum()) >= 1                       # an inversion piece was placed: mm_align1_inv's job was among them
    else:
        assert int(np.sum((cigs & 0xf) == 3)) >= 16


def test_the_switch_overrides_the_environment(H):
    assert not H.wm_ll_device_enabled()
    os.environ["WM_LL_DEV"] = "1"
    assert H.wm_ll_device_enabled()
    H.wm_set_ll_device(0)
    assert not H.wm_ll_device_enabled()
    H.wm_set_ll_device(-1)
    assert H.wm_ll_device_enabled()
    os.environ["WM_LL_DEV"] = "0"
    assert not H.wm_ll_device_enabled()
    H.wm_set_ll_device(1)
    assert H.wm_ll_device_enabled()


@pytest.mark.parametrize("combo", range(16))
def test_every_combination_with_the_sibling_switches_gives_the_same_text(H, INPUTS, combo):
    run = INPUTS["inversion"]
    reads = run["reads"][:3]
    fl = F_CIGAR | F_CG | F_EQX | F_CS
    for s in SIBLINGS + ("ll",):
        getattr(H, "wm_set_%s_device" % s)(0)
    want = map_text(H, run["h"], run["preset"], reads, fl)
    for k, s in enumerate(SIBLINGS):
        getattr(H, "wm_set_%s_device" % s)(combo >> k & 1)
    stats(H, True)
    H.wm_set_ll_device(1)
    assert map_text(H, run["h"], run["preset"], reads, fl) == want, combo
    assert stats(H)["deferred"] > 0

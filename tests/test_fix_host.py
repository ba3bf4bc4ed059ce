"""CPU: the host mapper with BOTH halves of mm_update_extra deferred (wm_set_fix_device(1): a region keeps its stitched CIGAR; mm_fix_cigar and the scan are one
batched request per read, served here by the default DeviceOps::fix_extra_batch — the specification of csrc/cigar_fix.h and the host walk) must reproduce the golden
fixtures and give exactly what it gives with the switch off, in splice mode too; wm_fix_stats counts what it did, among it the regions that took the host fix early
because mm_align1_inv was about to read their coordinates. With the switch unset nothing is deferred."""
import ctypes as C
import os
import tempfile
import numpy as np
import pytest
import wmtest as W
import e2e_common as E
from winnowmap_amd import build, synth

NAMES = ("deferred", "on_device", "on_host", "early_on_host", "calls", "device_us", "columns")


@pytest.fixture(scope="module")
def H():
    L = C.CDLL(build.build_harness())
    L.h_index_build_flag.restype = C.c_void_p
    L.h_index_build_flag.argtypes = [C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.c_int]
    L.h_map.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_char_p, C.c_int, C.c_char_p, W.i32p, C.c_int, W.u32p, C.c_int64, C.POINTER(C.c_int64), W.u64p]
    for f in (L.wm_fix_stats, L.wm_extra_stats):
        f.argtypes = [W.u64p, C.c_int]; f.restype = None
    for f in (L.wm_set_fix_device, L.wm_set_extra_device):
        f.argtypes = [C.c_int]; f.restype = None
    L.wm_fix_device_enabled.restype = C.c_int
    return L


@pytest.fixture(autouse=True)
def switch_back(H):
    saved = {k: os.environ.pop(k, None) for k in ("WM_FIX_DEV", "WM_EXTRA_DEV")}
    H.wm_set_fix_device(-1); H.wm_set_extra_device(-1)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
        H.wm_set_fix_device(-1); H.wm_set_extra_device(-1)
        stats(H, True)


def stats(H, reset=False):
    out = np.zeros(7, np.uint64)
    H.wm_fix_stats(out, 1 if reset else 0)
    return dict(zip(NAMES, (int(v) for v in out)))


def extra_stats(H, reset=False):
    out = np.zeros(6, np.uint64)
    H.wm_extra_stats(out, 1 if reset else 0)
    return [int(v) for v in out]


def map_reads(H, h, preset, reads):
    hits, cigs, first = [], [], [0]
    for i, s in enumerate(reads):
        ho = np.zeros(16 * 256, np.int32); co = np.zeros(2000000, np.uint32); nc = C.c_int64(); st = np.zeros(4, np.uint64)
        n = H.h_map(h, preset.encode(), 0x4 | 0x20, s, len(s), ("read%d" % i).encode(), ho, 256, co, len(co), C.byref(nc), st)
        assert n >= 0
        hits.append(ho[:16 * n].reshape(-1, 16).copy()); cigs.append(co[:nc.value].copy()); first.append(first[-1] + n)
    return np.concatenate(hits), np.concatenate(cigs), np.array(first, np.int64)


@pytest.mark.parametrize("name", ["ont", "hifi", "asm20", "ont_hpc", "ont_short"])
def test_both_halves_deferred_through_the_default_fix_extra_batch_match_the_golden(H, name):
    tmp = tempfile.mkdtemp()
    preset, fa, kf, k, reads = E.make_golden.inputs(name, tmp)
    h = H.h_index_build_flag(fa.encode(), (kf or "").encode(), k, 50, E.make_golden.IDX_FLAG.get(name, 0), 4)
    assert h
    stats(H, True); extra_stats(H, True)
    assert not H.wm_fix_device_enabled()
    hits0, cigs0, first0 = map_reads(H, h, preset, reads)
    assert not any(stats(H).values()) and not any(extra_stats(H))          # the variable unset: nothing is deferred, the parent's path
    E.compare(name, hits0, cigs0, first0, reads)
    os.environ["WM_FIX_DEV"] = "1"                                        # (read when a mapping call starts)
    assert H.wm_fix_device_enabled()
    hits, cigs, first = map_reads(H, h, preset, reads)
    st = stats(H); xs = extra_stats(H)
    E.compare(name, hits, cigs, first, reads)
    assert np.array_equal(hits, hits0) and np.array_equal(cigs, cigs0) and np.array_equal(first, first0)
    # every region with a CIGAR kept its stitched CIGAR; the oracle-backed ops have no device form, so the default fixed and walked them on the host — but for the
    # neighbours of an inversion test, which were fixed where the test ran and whose scan went through the scan-only queue
    assert st["deferred"] > 0 and st["on_device"] == 0 and st["calls"] == 0 and st["on_host"] + st["early_on_host"] == st["deferred"], st
    assert xs[0] == xs[2] == st["early_on_host"] and xs[1] == 0, (st, xs)
    assert st["deferred"] >= int((hits[:, 7] > 0).sum())


def test_an_inversion_test_fixes_its_two_neighbours_on_the_host_first(H):
    """reads with an inverted stretch: mm_align1_inv reads qs / qe / rs / re of the piece with split_inv and of the piece in front, which mm_fix_cigar may have
    moved; with the switch on both get the host fix there and then (counted), and the output does not move"""
    rng = np.random.default_rng(17)
    ref = synth.make_reference(1, 120000, 23, repeat_frac=0.0)
    tmp = tempfile.mkdtemp()
    fa = os.path.join(tmp, "inv.fa")
    synth.write_fasta(fa, ref)
    reads = []
    for i in range(6):
        p = int(rng.integers(2000, 90000))
        r = ref[0][p:p + 9000].copy()
        a = int(rng.integers(3000, 4000)); ln = int(rng.integers(600, 1500))
        r[a:a + ln] = synth.revcomp_codes(r[a:a + ln])
        for q in rng.integers(0, len(r), 90):                              # a few substitutions
            r[q] = (r[q] + 1) % 4
        reads.append(synth.codes_to_ascii(r))
    h = H.h_index_build_flag(fa.encode(), b"", 15, 50, 0, 4)
    assert h
    H.wm_set_fix_device(0)
    stats(H, True)
    hits0, cigs0, first0 = map_reads(H, h, "map-ont", reads)
    assert not any(stats(H).values())
    H.wm_set_fix_device(1)
    hits, cigs, first = map_reads(H, h, "map-ont", reads)
    st = stats(H)
    assert np.array_equal(hits, hits0) and np.array_equal(cigs, cigs0) and np.array_equal(first, first0)
    assert st["early_on_host"] >= 2 and st["on_host"] + st["early_on_host"] == st["deferred"], st


def test_splice_mode_gives_the_same_with_the_switch_on(H):
    ref = synth.make_reference(2, 200000, 191, repeat_frac=0.05)
    reads = [synth.codes_to_ascii(r) for r in synth.make_transcripts(ref, 16, 192)]
    tmp = tempfile.mkdtemp()
    fa = os.path.join(tmp, "ref.fa")
    synth.write_fasta(fa, ref)
    h = H.h_index_build_flag(fa.encode(), b"", 15, 25, 0, 4)
    assert h
    H.wm_set_fix_device(0)
    hits0, cigs0, first0 = map_reads(H, h, "splice", reads)
    H.wm_set_fix_device(1)
    stats(H, True)
    hits, cigs, first = map_reads(H, h, "splice", reads)
    st = stats(H)
    assert np.array_equal(hits, hits0) and np.array_equal(cigs, cigs0) and np.array_equal(first, first0)
    assert int(np.sum((cigs & 0xf) == 3)) >= 16 and len(hits) >= 16
    # (both transcript strands are aligned and one pass is dropped: only the kept one counts)
    assert st["deferred"] >= len(hits) and st["on_host"] + st["early_on_host"] == st["deferred"] and st["on_device"] == 0


def test_the_switch_overrides_the_environment(H):
    os.environ["WM_FIX_DEV"] = "1"
    H.wm_set_fix_device(0)
    assert not H.wm_fix_device_enabled()
    H.wm_set_fix_device(-1)
    assert H.wm_fix_device_enabled()
    os.environ["WM_FIX_DEV"] = "0"
    assert not H.wm_fix_device_enabled()
    H.wm_set_fix_device(1)
    assert H.wm_fix_device_enabled()

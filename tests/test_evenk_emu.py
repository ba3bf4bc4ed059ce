"""Even k without a GPU: (1) the oracle's mm_sketch against the reference's at even k without -H — the yardstick of everything below —, (2) the
one-wavefront-per-sequence sketch for even k (csrc/sketch_kernel.h: sketch_even_steps + the two phases over the surviving steps) on the wavefront
emulator against the oracle. Inputs: tests/evenkcases.py, on which the palindrome rule of src/sketch.c:166 fires often, also right behind an N."""
import ctypes as C
import tempfile
import numpy as np
import pytest
import wmtest as W
import evenkcases as EK
from winnowmap_amd import build, synth


def _need_ref():
    if not W.have_ref():
        build.build_oracle()                   # (builds oracle/_ref where the reference's sources are at hand)
    if not W.have_ref():
        pytest.skip("oracle/_ref not built (the reference's sources are not here)")


@pytest.mark.parametrize("w,k", EK.PAIRS)
def test_oracle_sketch_equals_reference_at_even_k(w, k):
    """wmo_sketch == mm_sketch at even k, plain (only -H with k = 14 was pinned so far): reference index with a matching-k -W list, so that the
    weighted order is in play; sequences with planted palindromes, microsatellites and N; lower case as well."""
    _need_ref()
    d = tempfile.mkdtemp()
    ref = EK.reference(3 + k)
    synth.write_fasta(d + "/ref.fa", ref)
    km, cnt = synth.repetitive_kmers(ref, k)
    synth.write_kmer_list(d + "/rep.txt", km, cnt, k)
    mi = W.ref().refshim_idx_build((d + "/ref.fa").encode(), (d + "/rep.txt").encode(), k, w, 2)
    f = W.o_bloom(km)
    seqs = EK.make_cases(w, k) + [ref[0][:20000], ref[1][40000:52000]]
    EK.assert_exercises_rule(seqs, k)
    n_mini = 0
    for i, s in enumerate(seqs):
        a = synth.codes_to_ascii(s)
        a = a.lower() if i % 5 == 0 else a
        ox, oy = W.o_sketch(a, w, k, rid=3, bloom=f)
        rx, ry = W.r_sketch(mi, a, w, k, rid=3)
        assert np.array_equal(ox, rx) and np.array_equal(oy, ry), (i, len(s))
        n_mini += len(ox)
    assert n_mini > 100
    W.ref().refshim_idx_destroy(mi)
    W.oracle().wmo_bloom_free(f)


@pytest.fixture(scope="module")
def emu():
    E = C.CDLL(build.build_emu_evenk())
    E.emu_evenk_sketch.argtypes = [C.c_int, W.u8p, W.u64p, W.i32p] + [C.c_int] * 4 + [C.c_uint32] * 3 + [W.u8p, W.u64p, W.u64p, W.u64p, W.i32p, W.i32p]
    E.emu_evenk_events.argtypes = [C.POINTER(C.c_longlong)]
    return E


def _emu_sketch(E, seqs, w, k, hpc, packed, tb, salts, bits):
    lens = np.array([len(s) for s in seqs], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    caps = (lens + 1).astype(np.int32)
    ooffs = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
    ox = np.zeros(int(caps.sum()), np.uint64); oy = np.zeros(int(caps.sum()), np.uint64); counts = np.zeros(len(seqs), np.int32)
    E.emu_evenk_sketch(len(seqs), np.concatenate(seqs), offs, lens, w, k, hpc, packed, tb, salts[0], salts[1], bits, ox, oy, ooffs, caps, counts)
    return [(ox[int(o):int(o) + n], oy[int(o):int(o) + n]) for o, n in zip(ooffs, counts)]


@pytest.fixture(scope="module")
def blooms():
    """per k: the oracle's filter of a -W list (so that the weighted order is in play) and its bit table for the kernel"""
    out = {}

    def get(k):
        if k not in out:
            km, _ = synth.repetitive_kmers(EK.reference(5, 2, 30000, 30), k)
            f = W.o_bloom(km)
            out[k] = (f,) + W.o_bloom_view(f)
        return out[k]
    return get


@pytest.mark.parametrize("hpc", [0, 1])
@pytest.mark.parametrize("w,k", EK.PAIRS)
def test_even_k_sketch_emulated_matches_oracle(emu, blooms, w, k, hpc):
    """sketch_coop at even k == the oracle, minimizer for minimizer, staged bytes and packed reads, with and without homopolymer compression; the event
    counters show that steps were skipped, some of them while fewer than k steps had survived since the last N."""
    f, tb, salts, bits = blooms(k)
    seqs = EK.make_cases(w, k)
    EK.assert_exercises_rule(seqs, k, bool(hpc))
    exp = [W.o_sketch(bytes(s), w, k, rid=0, bloom=f, hpc=bool(hpc)) for s in seqs]
    at = len(seqs) - 1                                  # all (AT): no minimizer at all — every step from the k-th on is skipped, l never reaches k
    assert len(exp[at][0]) == 0
    for packed in (0, 1):
        emu.emu_evenk_events_clear()
        got = _emu_sketch(emu, seqs, w, k, hpc, packed, tb, salts, bits)
        for i, ((gx, gy), (ex, ey)) in enumerate(zip(got, exp)):
            assert len(gx) == len(ex), (i, len(seqs[i]), packed, len(gx), len(ex))
            assert np.array_equal(gx, ex) and np.array_equal(gy, ey), (i, len(seqs[i]), packed)
        ev = (C.c_longlong * 2)()
        emu.emu_evenk_events(ev)
        st = np.array([EK.skip_stats(s, k, bool(hpc)) for s in seqs]).sum(axis=0)
        assert ev[0] > 0 and ev[1] > 0, (ev[0], ev[1])
        assert ev[0] == st[1], (ev[0], [int(x) for x in st])            # (the kernel skipped exactly the steps the restated rule skips)
    assert sum(len(e[0]) for e in exp) > 100


@pytest.mark.parametrize("hpc", [0, 1])
def test_odd_k_is_untouched(emu, blooms, hpc):
    """one odd k through the same entry: identical to the oracle, and not one step is skipped"""
    w, k = 10, 15
    f, tb, salts, bits = blooms(k)
    seqs = EK.make_cases(w, 14)
    emu.emu_evenk_events_clear()
    for packed in (0, 1):
        got = _emu_sketch(emu, seqs, w, k, hpc, packed, tb, salts, bits)
        for i, s in enumerate(seqs):
            ex, ey = W.o_sketch(bytes(s), w, k, rid=0, bloom=f, hpc=bool(hpc))
            assert np.array_equal(got[i][0], ex) and np.array_equal(got[i][1], ey), (i, packed)
    ev = (C.c_longlong * 2)()
    emu.emu_evenk_events(ev)
    assert ev[0] == 0 and ev[1] == 0

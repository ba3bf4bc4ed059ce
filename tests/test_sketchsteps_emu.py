"""The chunked sketch of long sequences under -H and at an even k without a GPU (csrc/sketch_kernel.h: sketch_steps_stage / sketch_steps_scan, then the two
phases over slot space; tests/simt_emu/emu_sketchsteps.cpp runs them one emulated wavefront per chunk in launch order): bit for bit the oracle's mm_sketch and the
one-wavefront-per-sequence form, at chunk sizes small enough that runs, (AT)n arrays, N runs and low-complexity stretches span several chunks. The oracle's
sketch is pinned to the reference's at these k and under -H by tests/test_evenk_emu.py and tests/test_oracle_vs_ref.py."""
import ctypes as C
import numpy as np
import pytest
import wmtest as W
import evenkcases as EK
from winnowmap_amd import build, synth

MODES = ((1, 15), (0, 14), (1, 14), (1, 16), (0, 2))                    # (hpc, k)
WS = (10, 50)
CHUNKS = (64, 65, 200, 1000)
AT = np.array([0, 3], np.uint8)


@pytest.fixture(scope="module")
def emu():
    E = C.CDLL(build.build_emu_sketchsteps())
    E.emu_sketchsteps.argtypes = [C.c_int, W.u8p, W.u64p, W.i32p] + [C.c_int] * 4 + [C.c_uint32] * 3 + [W.u8p, W.u64p, W.u64p, W.u64p, W.i32p, W.i32p, C.c_int, W.i32p, W.u64p]
    O = C.CDLL(build.build_emu_evenk())
    O.emu_evenk_sketch.argtypes = [C.c_int, W.u8p, W.u64p, W.i32p] + [C.c_int] * 4 + [C.c_uint32] * 3 + [W.u8p, W.u64p, W.u64p, W.u64p, W.i32p, W.i32p]
    return E, O


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


def _layout(seqs):
    lens = np.array([len(s) for s in seqs], np.int32)
    offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
    caps = (lens + 1).astype(np.int32)
    ooffs = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
    flat = np.ascontiguousarray(np.concatenate(seqs + [np.zeros(1, np.uint8)]), np.uint8)       # (never empty)
    return lens, offs, caps, ooffs, flat


def _chunked(E, seqs, w, k, hpc, packed, chunk, bl):
    """-> per sequence (x, y), per sequence its chunks' (begin, end, sync) in slot space"""
    _, tb, salts, bits = bl
    lens, offs, caps, ooffs, flat = _layout(seqs)
    n_ch = np.maximum(1, (lens + chunk - 1) // chunk)
    roffs = np.concatenate([[0], np.cumsum(n_ch)[:-1]]).astype(np.uint64)
    ranges = np.full(3 * int(n_ch.sum()), -99, np.int32)
    ox = np.zeros(int(caps.sum()), np.uint64); oy = np.zeros(int(caps.sum()), np.uint64); counts = np.zeros(len(seqs), np.int32)
    assert E.emu_sketchsteps(len(seqs), flat, offs, lens, w, k, hpc, packed, tb, salts[0], salts[1], bits, ox, oy, ooffs, caps, counts, chunk, ranges, roffs) == 0
    ranges = ranges.reshape(-1, 3)
    return ([(ox[int(o):int(o) + n], oy[int(o):int(o) + n]) for o, n in zip(ooffs, counts)],
            [ranges[int(o):int(o) + int(m)] for o, m in zip(roffs, n_ch)])


def _one_wave(O, seqs, w, k, hpc, packed, bl):
    _, tb, salts, bits = bl
    lens, offs, caps, ooffs, flat = _layout(seqs)
    ox = np.zeros(int(caps.sum()), np.uint64); oy = np.zeros(int(caps.sum()), np.uint64); counts = np.zeros(len(seqs), np.int32)
    O.emu_evenk_sketch(len(seqs), flat, offs, lens, w, k, hpc, packed, tb, salts[0], salts[1], bits, ox, oy, ooffs, caps, counts)
    return [(ox[int(o):int(o) + n], oy[int(o):int(o) + n]) for o, n in zip(ooffs, counts)]


def _oracle(seqs, w, k, hpc, bl):
    return [W.o_sketch(bytes(s), w, k, rid=0, bloom=bl[0], hpc=bool(hpc)) if len(s) else (np.zeros(0, np.uint64),) * 2 for s in seqs]


def _check(got, exp, what):
    for i, ((gx, gy), (ex, ey)) in enumerate(zip(got, exp)):
        assert len(gx) == len(ex), what + (i, len(gx), len(ex))
        assert np.array_equal(gx, ex) and np.array_equal(gy, ey), what + (i,)


def _stats(ranges):
    """(chunks whose slot range is empty, chunks behind the first that hold slots but no sync position: absorbed by their predecessor)"""
    empty = sum(int((r[:, 0] == r[:, 1]).sum()) for r in ranges)
    absorbed = sum(int(((r[1:, 1] > r[1:, 0]) & (r[1:, 2] < 0)).sum()) for r in ranges)
    return empty, absorbed


def constructed(w, k, C_, rng):
    """name -> sequence; C_: the chunk size the boundaries are laid out for"""
    R = lambda n: synth.random_codes(n, rng)      # noqa: E731
    out = {}
    out["run_over_3_chunks"] = np.concatenate([R(300), np.full(3 * C_ + 50, 0), R(300)])
    at = np.tile(AT, (4 * C_ + 50) // 2)
    at[len(at) // 2:len(at) // 2 + 2] = 4                                # (two bases: the array keeps its phase behind the N)
    out["at_over_3_chunks"] = np.concatenate([R(300), at, R(300)])
    s = R(2 * C_ + 100)
    s[C_ - 3:C_ + 4] = 2
    out["boundary_in_run"] = s
    # an (AT)n array around the boundary at 2 C_ with a two-base N that ends k - 1 codes before the boundary: the steps on both sides of it are palindromes
    # whose test reads across the N run and across the boundary
    s = R(3 * C_ + 40)
    s[2 * C_ - 40:2 * C_ + 40] = np.tile(AT, 40)
    s[2 * C_ - (k - 1) - 2:2 * C_ - (k - 1)] = 4
    out["boundary_k1_after_N"] = s
    lead = (-300) % C_ + C_                                              # runs of 40 bases, a boundary in their middle: any k of them span >= 256 bases
    out["long_span_over_boundary"] = np.concatenate([R(lead), np.repeat(np.tile(np.arange(4), 4)[:15], 40), R(300)])
    out["all_N_chunk"] = np.concatenate([R(C_ + 10), np.full(2 * C_, 4), R(C_)])
    out["no_sync_two_chunks"] = np.concatenate([R(C_ + 30), np.tile(np.array([0, 1], np.uint8), (5 * C_) // 4), R(C_)])      # (AC)n over 2.5 chunks: two k-mers in turn, never a strict minimum
    out["fewer_slots_than_w"] = R(7)
    out["fewer_slots_than_w_many_chunks"] = np.concatenate([np.full(2 * C_ + 9, 1), R(5)])
    out["no_slot"] = np.zeros(0, np.uint8)
    out["all_N"] = np.full(2 * C_ + 3, 4)
    return {n_: np.ascontiguousarray(v, np.uint8) for n_, v in out.items()}


@pytest.mark.parametrize("w", WS)
@pytest.mark.parametrize("hpc,k", MODES)
def test_chunked_steps_equal_oracle_and_one_wavefront(emu, blooms, hpc, k, w):
    E, O = emu
    bl = blooms(k)
    base = EK.make_cases(w, k - (k & 1))                # (k = 15: the inputs made for 14)
    exp_base = _oracle(base, w, k, hpc, bl)
    assert sum(len(e[0]) for e in exp_base) > 100
    for pk_ in (0, 1):
        _check(_one_wave(O, base, w, k, hpc, pk_, bl), exp_base, ("one wavefront", hpc, k, w, pk_))
    rng = np.random.default_rng(100 * k + w + hpc)
    for ci, chunk in enumerate(CHUNKS):
        _check(_chunked(E, base, w, k, hpc, ci & 1, chunk, bl)[0], exp_base, ("chunked", hpc, k, w, chunk))
        cs = constructed(w, k, chunk, rng)
        names, seqs = list(cs), list(cs.values())
        exp = _oracle(seqs, w, k, hpc, bl)
        assert len(exp[names.index("no_slot")][0]) == 0 and len(exp[names.index("fewer_slots_than_w")][0]) <= 1
        one = _one_wave(O, seqs, w, k, hpc, 0, bl)
        _check(one, exp, ("one wavefront, constructed", hpc, k, w, chunk))
        for pk_ in (0, 1):
            got, ranges = _chunked(E, seqs, w, k, hpc, pk_, chunk, bl)
            _check(got, exp, ("chunked, constructed", hpc, k, w, chunk, pk_))
            rg = dict(zip(names, ranges))
            if hpc:                                                      # chunks inside the run hold no step end
                assert int((rg["run_over_3_chunks"][:, 0] == rg["run_over_3_chunks"][:, 1]).sum()) >= 2, rg["run_over_3_chunks"]
                assert 0 < rg["fewer_slots_than_w_many_chunks"][-1][1] < w and len(rg["fewer_slots_than_w_many_chunks"]) >= 3
            if not k & 1:                                                # chunks inside the array have no survivor
                assert int((rg["at_over_3_chunks"][:, 0] == rg["at_over_3_chunks"][:, 1]).sum()) >= 2, rg["at_over_3_chunks"]
            assert rg["no_slot"].tolist() == [[0, 0, 0]]
            # the (AC)n stretch: at least one chunk that holds slots is absorbed
            r = rg["no_sync_two_chunks"]
            assert int(((r[1:, 1] > r[1:, 0]) & (r[1:, 2] < 0)).sum()) >= 1, r


def fuzz_sequences(seed, n=300):
    rng = np.random.default_rng(seed)
    seqs = []
    for _ in range(n):
        s = synth.random_codes(int(rng.integers(200, 5001)), rng)
        for _ in range(int(rng.integers(0, 4))):                         # homopolymer runs
            m = int(rng.integers(5, 601)); p = int(rng.integers(0, len(s)))
            s[p:p + m] = rng.integers(0, 4)
        for _ in range(int(rng.integers(0, 4))):                         # (AT)n / (CG)n arrays, some with an N inside
            m = int(rng.integers(20, 601)); p = int(rng.integers(0, len(s)))
            a = np.tile(np.array(((0, 3), (3, 0), (1, 2), (2, 1))[int(rng.integers(0, 4))], np.uint8), m // 2 + 1)[:len(s[p:p + m])]
            if len(a) > 4 and rng.random() < 0.5:
                q = int(rng.integers(0, len(a) - 2))
                a[q:q + int(rng.integers(1, 3))] = 4
            s[p:p + m] = a
        for _ in range(int(rng.integers(0, 4))):                         # N: a base or three, now and then a long run
            m = int(rng.integers(1, 4)) if rng.random() < 0.8 else int(rng.integers(20, 300)); p = int(rng.integers(0, len(s)))
            s[p:p + m] = 4
        seqs.append(np.ascontiguousarray(s, np.uint8))
    return seqs


@pytest.mark.parametrize("hpc,k", MODES)
def test_fuzz_chunked_steps(emu, blooms, hpc, k):
    """300 random sequences of 200 - 5 000 codes with implanted runs, (AT)n arrays and N, half of them at w = 10 and half at w = 50, at every chunk size; the
    returned ranges show that chunks with an empty slot range and absorbed chunks both occurred"""
    E, _ = emu
    bl = blooms(k)
    seqs = fuzz_sequences(7000 + 10 * k + hpc)
    half = len(seqs) // 2
    empty = absorbed = n_mini = 0
    for w, part in ((10, seqs[:half]), (50, seqs[half:])):
        exp = _oracle(part, w, k, hpc, bl)
        n_mini += sum(len(e[0]) for e in exp)
        for ci, chunk in enumerate(CHUNKS):
            got, ranges = _chunked(E, part, w, k, hpc, (ci + hpc) & 1, chunk, bl)
            _check(got, exp, ("fuzz", hpc, k, w, chunk))
            e_, a_ = _stats(ranges)
            empty += e_; absorbed += a_
    print("hpc %d k %d: %d minimizers; chunks with an empty slot range %d, absorbed %d" % (hpc, k, n_mini, empty, absorbed))
    assert n_mini > 1000 and empty >= 1 and absorbed >= 1, (n_mini, empty, absorbed)

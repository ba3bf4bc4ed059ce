"""The -T filter on the CPU: the two kernels of csrc/sdust_kernel.h on the host wavefront emulator and the host restatement (csrc/host/wm_sdust.h)
against the reference's own sdust() (src/sdust.c:166, taken from oracle/_ref/libwinnowmap_ref.so) with W = 64 as mm_dust_minier calls it
(src/map.c:50), and the squeeze of the minimizers against src/map.c:51-63 restated in sdustcases.restated_filter. Every comparison is exact."""
import ctypes as C
import ctypes.util
import numpy as np
import pytest
import wmtest as W
import sdustcases as S
from winnowmap_amd import build

pytestmark = pytest.mark.skipif(not W.have_ref(), reason="oracle/_ref not built")

libc = C.CDLL(ctypes.util.find_library("c") or "libc.so.6")
libc.free.argtypes = [C.c_void_p]
ASCII = np.frombuffer(b"ACGTN", np.uint8)


def _bind(path):
    E = C.CDLL(path)
    E.emu_sdust.argtypes = [W.u8p, C.c_int, C.c_int, C.c_int, W.i32p, C.c_int, W.i32p]
    E.host_sdust.argtypes = [W.u8p, C.c_int, C.c_int, W.i32p, C.c_int, W.i32p]
    E.emu_dust_filter.argtypes = [W.u64p, W.u64p, C.c_int, W.i32p, C.c_int]
    E.host_dust_filter.argtypes = [W.u64p, W.u64p, C.c_int, W.i32p, C.c_int]
    E.emu_dust_job.argtypes = [W.u8p, C.c_int, C.c_int, W.u64p, W.u64p, C.c_int, W.i32p]
    return E


@pytest.fixture(scope="module")
def emu():
    return _bind(build.build_emu_sdust())


@pytest.fixture(scope="module")
def ref_sdust():
    R = C.CDLL(W.REF_SO)
    R.sdust.restype = C.c_void_p
    R.sdust.argtypes = [C.c_void_p, C.c_char_p, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int)]

    def run(codes, T):
        n = C.c_int()
        text = ASCII[np.minimum(codes, 4)].tobytes()
        p = R.sdust(None, text, len(text), T, 64, C.byref(n))
        r = np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint64)), (n.value,)).copy() if n.value else np.zeros(0, np.uint64)
        libc.free(p)
        return [(int(v >> np.uint64(32)), int(v & np.uint64(0xffffffff))) for v in r]
    return run


def _emu_iv(E, codes, T, packed=0):
    codes = np.ascontiguousarray(codes, np.uint8)
    cap = len(codes) + 70
    iv = np.zeros(2 * cap + 2, np.int32)
    high = np.zeros(1, np.int32)
    n = E.emu_sdust(codes if len(codes) else np.zeros(1, np.uint8), len(codes), T, packed, iv, cap, high)
    return (None if n < 0 else [(int(iv[2 * i]), int(iv[2 * i + 1])) for i in range(n)]), int(high[0])


def _host_iv(E, codes, T):
    codes = np.ascontiguousarray(codes, np.uint8)
    cap = len(codes) + 70
    iv = np.zeros(2 * cap + 2, np.int32)
    high = np.zeros(1, np.int32)
    n = E.host_sdust(codes if len(codes) else np.zeros(1, np.uint8), len(codes), T, iv, cap, high)
    assert n <= cap
    return [(int(iv[2 * i]), int(iv[2 * i + 1])) for i in range(n)], int(high[0])


def _flat(iv):
    return np.array([v for p in iv for v in p] + [0, 0], np.int32)


HIGH = {"emu": 0}


@pytest.mark.parametrize("T", S.THRESHOLDS)
def test_intervals_named_cases(emu, ref_sdust, T):
    masked = 0
    for name, codes in S.named_cases():
        want = ref_sdust(codes, T)
        for packed in (0, 1):
            got, high = _emu_iv(emu, codes, T, packed)
            assert got == want, (name, T, packed, got, want)
        host, hhigh = _host_iv(emu, codes, T)
        assert host == want, (name, T, host, want)
        assert hhigh == high, (name, T, hhigh, high)              # both keep the same list
        masked += len(want)
        HIGH["emu"] = max(HIGH["emu"], high)
    assert masked > 50


def test_the_list_of_perfect_intervals_grows_into_the_thousands(emu, ref_sdust):
    """the state that survives an ambiguous base: intervals past the bases read so far and a list far beyond one window's 62 suffixes"""
    codes = S.p_list_stress(np.random.default_rng(20))
    got, high = _emu_iv(emu, codes, 20)
    want = ref_sdust(codes, 20)
    assert got == want
    assert want == [(300, 501), (601, 681)], want              # (the dinucleotide run 300..499 and the homopolymer 601..680 behind the N at 600)
    assert 1000 < high <= 4096, high


@pytest.mark.parametrize("part", range(4))
def test_intervals_random_mixtures(emu, ref_sdust, part):
    n_iv = 0
    for seed in range(part, S.N_MIXTURES, 4):
        codes = S.mixture(seed)
        assert len(codes) <= 1500
        for T in S.THRESHOLDS:                                  # the host restatement at every threshold, the emulated wavefront at one (it is ~100 x slower)
            want = ref_sdust(codes, T)
            host, high = _host_iv(emu, codes, T)
            assert host == want, (seed, T, host, want)
            if T == S.THRESHOLDS[(seed >> 2) & 3]:
                got, ehigh = _emu_iv(emu, codes, T, seed & 1)
                assert got == want and ehigh == high, (seed, T, got, want, ehigh, high)
            n_iv += len(want)
            HIGH["emu"] = max(HIGH["emu"], high)
    print("largest list of perfect intervals so far: %d" % HIGH["emu"])
    assert n_iv > 100 and HIGH["emu"] <= 4096


@pytest.mark.parametrize("hpc", (False, True))
def test_filter_against_the_restated_loop(emu, ref_sdust, hpc):
    rng = np.random.default_rng(5 + int(hpc))
    dropped = kept = back = 0
    cases = [c for _, c in S.named_cases()] + [S.mixture(s) for s in range(0, S.N_MIXTURES, 5)] + [S.long_case()[:9000]]
    for ci, codes in enumerate(cases):
        for T in (20, 4):
            iv = ref_sdust(codes, T)
            dens = (3, 8, 20)[ci % 3]                                  # sparse as w = 50 leaves them, and dense: several steps of 64 with overlapping spans
            mx, my = S.minimizers(rng, len(codes), len(codes) // dens, hpc)
            want = S.restated_filter(mx, my, iv)
            s = ((my & np.uint64(0xffffffff)) >> np.uint64(1)).astype(np.int64) - (mx & np.uint64(0xff)).astype(np.int64)
            back += int(hpc and len(s) > 1 and bool((np.diff(s) < 0).any()))
            for fn in (emu.emu_dust_filter, emu.host_dust_filter):
                gx, gy = mx.copy(), my.copy()
                k = fn(gx if len(gx) else np.zeros(1, np.uint64), gy if len(gy) else np.zeros(1, np.uint64), len(mx), _flat(iv), len(iv))
                assert k == len(want) and np.array_equal(gx[:k], mx[want]) and np.array_equal(gy[:k], my[want]), (ci, T, hpc, k, len(want))
            dropped += len(mx) - len(want)
            kept += len(want)
    assert dropped > 200 and kept > 200 and (back > 20 or not hpc), (dropped, kept, back)


def test_forced_overflow_is_finished_by_the_host(ref_sdust):
    """the list compiled down to 64 entries: the wavefront gives up, the host restatement finishes the job, the result is the reference's"""
    E = _bind(build.build_emu_sdust(("WM_SDUST_CAP=64",)))
    assert E.emu_sdust_cap() == 64
    rng = np.random.default_rng(3)
    fell = 0
    for name, codes in [("p_list_stress", S.p_list_stress(np.random.default_rng(20)))] + S.named_cases()[20:60:3]:
        codes = np.ascontiguousarray(codes)
        iv = ref_sdust(codes, 20)
        mx, my = S.minimizers(rng, len(codes), len(codes) // 6, True)
        want = S.restated_filter(mx, my, iv)
        fb = np.zeros(1, np.int32)
        gx, gy = mx.copy(), my.copy()
        k = E.emu_dust_job(codes, len(codes), 20, gx if len(gx) else np.zeros(1, np.uint64), gy if len(gy) else np.zeros(1, np.uint64), len(mx), fb)
        assert k == len(want) and np.array_equal(gx[:k], mx[want]) and np.array_equal(gy[:k], my[want]), (name, k, len(want))
        fell += int(fb[0])
        if name == "p_list_stress":
            assert fb[0] == 1 and _emu_iv(E, codes, 20)[0] is None
    assert fell >= 1
